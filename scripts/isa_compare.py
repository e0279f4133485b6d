"""Compare the gfx950 instruction streams of the kernels of two source trees.

    python scripts/isa_compare.py <tree A> <tree B> [--title TEXT] [--files-a F,F,...] [--files-b F,F,...]   (markdown on stdout)

Compiles the named files of csrc/ (by default csrc/gs2d*.hip, gs2d_maps.hip apart, and csrc/gs3d_pergaussian.hip; --files-b
defaults to --files-a) of both trees to assembly with the command line of tests/test_kernel_resources.py (the library's flags plus --cuda-device-only -S), splits the text per kernel
symbol, drops directives and comments, and reports per kernel whether the instruction sequence is identical, a
permutation, or different, next to the compiler's resource summary of both sides.  A kernel that is different but
becomes a permutation once register numbers are masked is reported as "permuted, registers renamed": that is NOT a
permutation, only the mildest kind of difference.  It compares text only.  Basic-block labels carry the ordinal of the
function within its file, which a move between files changes: they are renumbered per kernel in order of appearance
before the comparison.  Kernels are matched by symbol.  A kernel of a shared header exists once per file that includes
it: such copies are matched by file name, and a copy whose file the other tree does not have against the other tree's
first copy."""
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


def sources(tree, names=None):
    csrc = os.path.join(tree, "scorp_amd", "csrc")
    if names:
        return [os.path.join(csrc, n) for n in names]
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


def tree_kernels(tree, names=None):
    """{symbol: [(file, instructions, figures) of every file that has it]}"""
    with concurrent.futures.ThreadPoolExecutor(max_workers=4) as pool:
        srcs = sources(tree, names)
        texts = list(pool.map(lambda s: assembly(tree, s), srcs))
    out = {}
    for s, t in zip(srcs, texts):
        for k, v in kernels(t, os.path.basename(s)).items():
            out.setdefault(k, []).append(v)
    return out


def matched(a, b):
    """[(symbol, copy of A or None, copy of B or None)]"""
    rows = []
    for k in sorted(set(a) | set(b)):
        ca, cb = a.get(k, []), b.get(k, [])
        if not ca or not cb:
            rows += [(k, v, None) for v in ca] + [(k, None, v) for v in cb]
            continue
        by_file = {v[0]: v for v in cb}
        used = set()
        for v in ca:
            w = by_file.get(v[0], cb[0])
            used.add(w[0])
            rows.append((k, v, w))
        rows += [(k, ca[0], w) for w in cb if w[0] not in used]
    return rows


def option(name):
    return sys.argv[sys.argv.index(name) + 1].split(",") if name in sys.argv else None


def main():
    if len(sys.argv) < 3:
        sys.exit(__doc__)
    title = sys.argv[sys.argv.index("--title") + 1] if "--title" in sys.argv else "Instruction streams"
    files_a = option("--files-a")
    a, b = tree_kernels(sys.argv[1], files_a), tree_kernels(sys.argv[2], option("--files-b") or files_a)
    rows = matched(a, b)
    verdicts = collections.Counter()
    print(f"## {title}\n")
    print("| kernel | A | B | instructions A / B | sequence | " + " | ".join(FIGURES) + " |")
    print("|---|---|---|---|---|" + "---|" * len(FIGURES))
    for k, va, vb in rows:
        if va is None or vb is None:
            verdict = "only in A" if va else "only in B"
            fa = va or vb
            print(f"| `{k}` | {va[0] if va else '-'} | {vb[0] if vb else '-'} | - | {verdict} | " + " | ".join(str(fa[2].get(f)) for f in FIGURES) + " |")
            verdicts[verdict] += 1
            continue
        (fa, ia, ra), (fb, ib, rb) = va, vb
        verdict = verdict_of(ia, ib)
        if ra != rb:
            verdict += ", RESOURCES DIFFER"
        verdicts[verdict] += 1
        figs = " | ".join(str(ra.get(f)) if ra.get(f) == rb.get(f) else f"{ra.get(f)} -> {rb.get(f)}" for f in FIGURES)
        print(f"| `{k}` | {fa} | {fb} | {len(ia)} / {len(ib)} | {verdict} | {figs} |")
    print("\n" + ", ".join(f"{n} {v}" for v, n in sorted(verdicts.items())) + f" ({len(rows)} kernels).\n")


if __name__ == "__main__":
    main()
