"""Compare the gfx950 instruction streams of the per-primitive and surfel kernels of two source trees.

    python scripts/isa_compare.py <tree A> <tree B> [--title TEXT]      (markdown on stdout)

Compiles csrc/gs2d*.hip (gs2d_maps.hip apart) and csrc/gs3d_pergaussian.hip of both trees to assembly with the command
line of tests/test_kernel_resources.py (the library's flags plus --cuda-device-only -S), splits the text per kernel
symbol, drops directives and comments, and reports per kernel whether the instruction sequence is identical, a
permutation, or different, next to the compiler's resource summary of both sides.  A kernel that is different but
becomes a permutation once register numbers are masked is reported as "permuted, registers renamed": that is NOT a
permutation, only the mildest kind of difference.  It compares text only.  Basic-block labels carry the ordinal of the
function within its file, which a move between files changes: they are renumbered per kernel in order of appearance
before the comparison."""
import collections
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
from tests.test_kernel_resources import asm_command  # noqa: E402

FIGURES = ("NumVgprs", "TotalNumSgprs", "ScratchSize", "LDSByteSize", "Occupancy")   # (as the compiler's summary names them)


def sources(tree):
    csrc = os.path.join(tree, "scorp_amd", "csrc")
    files = [f for f in sorted(glob.glob(os.path.join(csrc, "gs2d*.hip"))) if os.path.basename(f) != "gs2d_maps.hip"]
    return files + [os.path.join(csrc, "gs3d_pergaussian.hip")]


def assembly(tree, src):
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "k.s")
        subprocess.run(asm_command(src, out, root=tree), check=True, stdout=subprocess.PIPE, stderr=subprocess.PIPE)
        return open(out).read()


def kernels(text, origin):
    """{symbol: (file, [instruction lines], {figure: value})}"""
    res, cur, body = {}, None, None
    for line in text.splitlines():
        m = re.match(r"^(_Z\w+):", line)
        if m:
            cur, body = m.group(1), []
            res[cur] = (origin, body, {})
            continue
        if cur is None:
            continue
        m = re.match(r"^; (\w+): (\d+)", line)
        if m and m.group(1) in FIGURES:
            res[cur][2][m.group(1)] = int(m.group(2))
            continue
        if body is None:
            continue
        if re.match(r"^\.Lfunc_end\d+:", line):
            body = None   # (the resource comments of this kernel follow)
            continue
        code = line.split(";", 1)[0].strip()
        if not code or (code.startswith(".") and not re.match(r"^\.LBB\d+_\d+:", code)):
            continue
        body.append(code)
    return {k: v for k, v in res.items() if v[2]}


def renumbered(body):
    names = {}
    def sub(m):
        return names.setdefault(m.group(0), f".L{len(names)}")
    return [re.sub(r"\.LBB\d+_\d+", sub, c) for c in body]


def unlabelled(body, registers=True):
    """The multiset of instructions, branch targets apart; registers=False: register numbers apart too."""
    out = [re.sub(r"\.LBB\d+_\d+", ".L", c) for c in body if not c.endswith(":")]
    if not registers:
        out = [re.sub(r"\b([vsa])(\d+|\[\d+:\d+\])", r"\1", c) for c in out]
    return collections.Counter(out)


def verdict_of(ia, ib):
    if renumbered(ia) == renumbered(ib):
        return "identical"
    if unlabelled(ia) == unlabelled(ib):
        return "permuted"
    if unlabelled(ia, False) == unlabelled(ib, False):
        return "permuted, registers renamed"   # (a difference: the same instructions with other register numbers)
    return "DIFFERENT"


def tree_kernels(tree):
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        srcs = sources(tree)
        texts = list(pool.map(lambda s: assembly(tree, s), srcs))
    out = {}
    for s, t in zip(srcs, texts):
        for k, v in kernels(t, os.path.basename(s)).items():
            assert k not in out, f"{k} in {out[k][0]} and {v[0]}"
            out[k] = v
    return out


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    title = sys.argv[sys.argv.index("--title") + 1] if "--title" in sys.argv else "Instruction streams"
    a, b = tree_kernels(sys.argv[1]), tree_kernels(sys.argv[2])
    verdicts = collections.Counter()
    print(f"## {title}\n")
    print("| kernel | A | B | instructions A / B | sequence | " + " | ".join(FIGURES) + " |")
    print("|---|---|---|---|---|" + "---|" * len(FIGURES))
    for k in sorted(set(a) | set(b)):
        if k not in a or k not in b:
            verdict = "only in A" if k in a else "only in B"
            fa = a.get(k, b.get(k))
            print(f"| `{k}` | {a[k][0] if k in a else '-'} | {b[k][0] if k in b else '-'} | - | {verdict} | " + " | ".join(str(fa[2].get(f)) for f in FIGURES) + " |")
            verdicts[verdict] += 1
            continue
        (fa, ia, ra), (fb, ib, rb) = a[k], b[k]
        verdict = verdict_of(ia, ib)
        if ra != rb:
            verdict += ", RESOURCES DIFFER"
        verdicts[verdict] += 1
        figs = " | ".join(str(ra.get(f)) if ra.get(f) == rb.get(f) else f"{ra.get(f)} -> {rb.get(f)}" for f in FIGURES)
        print(f"| `{k}` | {fa} | {fb} | {len(ia)} / {len(ib)} | {verdict} | {figs} |")
    print("\n" + ", ".join(f"{n} {v}" for v, n in sorted(verdicts.items())) + f" ({len(set(a) | set(b))} kernels).\n")


if __name__ == "__main__":
    main()
