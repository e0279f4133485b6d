"""The ctypes binding scorp_amd/_C.py derives from include/scorp_gs.h, compared with the hand-written tables of an earlier
commit's _C.py (profiles/abi_binding_equal.json).  No GPU and no built library: both modules' lib() run against a stand-in
for ctypes.CDLL that records the restype / argtypes set on each function.

    python scripts/dev/abi_binding_dump.py <parent commit> out.json

Per function: restype, the class of every argument (struct pointers by the struct's name); per struct: field names, field
classes, offsets, size; per constant of the parent: name and value.  The only differences allowed are the six host-pointer
arguments the parent typed POINTER(c_uint64 / c_uint64 * 3 / c_double) and the derived table types c_void_p; the exit status
is 1 for any other.  Also the import time of either module in a fresh interpreter (median), next to `import torch`."""
import ctypes
import importlib.util
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "..")
NEW_PATH = os.path.join(ROOT, "scorp_amd", "_C.py")
EXPECTED = {("scorp_gs3d_num_pairs", 2), ("scorp_gs3d_check_overflow", 2), ("scorp_gs3d_debug_work", 4),
            ("scorp_cloud_orient_normals", 5), ("scorp_pose_adam_9dof", 9), ("scorp_mesh_smooth", 5)}
LOAD = "import time, importlib.util as u; t = time.perf_counter(); s = u.spec_from_file_location('m', {!r}); " \
       "m = u.module_from_spec(s); s.loader.exec_module(m); print(time.perf_counter() - t)"


def load(path):
    spec = importlib.util.spec_from_file_location("abi_" + str(abs(hash(path))), path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class _Function:
    restype, argtypes = ctypes.c_int, None   # what ctypes assumes of a function nobody typed


class _Library:
    def __init__(self, path):
        self.functions = {}

    def __getattr__(self, name):
        if name.startswith("__"):
            raise AttributeError(name)
        return self.functions.setdefault(name, _Function())


def bound(mod):
    """{function: (restype, argtypes)} as mod.lib() sets them"""
    import torch  # noqa: F401  (lib() imports it, and it loads its own libraries with the real CDLL)
    real, ctypes.CDLL = ctypes.CDLL, _Library
    try:
        mod.LIB_PATH, mod._lib = NEW_PATH, None   # (any file that exists)
        functions = mod.lib().functions
        for name in mod.EXPORTS:   # an export lib() never touched is called with ctypes' defaults
            getattr(mod.lib(), name)
        return {k: (f.restype, f.argtypes) for k, f in functions.items()}
    finally:
        ctypes.CDLL, mod._lib = real, None


def describe(t):
    if isinstance(t, type) and issubclass(t, ctypes._Pointer):
        return f"POINTER({describe(t._type_)})"
    if isinstance(t, type) and issubclass(t, ctypes.Array):
        return f"{describe(t._type_)} * {t._length_}"
    return t.__name__


def structs_of(mod):
    return {k: v for k, v in vars(mod).items() if isinstance(v, type) and issubclass(v, ctypes.Structure) and v is not ctypes.Structure}


def layout(s):
    return [(n, describe(t), getattr(s, n).offset) for n, t in s._fields_] + [ctypes.sizeof(s)]


def import_seconds(path, runs=7):
    return statistics.median(float(subprocess.check_output([sys.executable, "-c", LOAD.format(path)])) for _ in range(runs))


def main(parent, out_path):
    with tempfile.TemporaryDirectory() as tmp:
        old_path = os.path.join(tmp, "parent_C.py")
        with open(old_path, "wb") as f:
            f.write(subprocess.check_output(["git", "-C", ROOT, "show", f"{parent}:scorp_amd/_C.py"]))
        old, new = load(old_path), load(NEW_PATH)
        seconds = {"parent": import_seconds(old_path), "derived": import_seconds(NEW_PATH)}
    seconds["import_torch"] = statistics.median(
        float(subprocess.check_output([sys.executable, "-c", "import time; t = time.perf_counter(); import torch; "
                                                             "print(time.perf_counter() - t)"])) for _ in range(3))
    fa, fb = bound(old), bound(new)
    expected, other = [], []
    for name in sorted(set(fa) | set(fb)):
        if name not in fa or name not in fb:
            other.append(f"{name}: bound by {'the parent' if name in fa else 'the derived table'} only")
            continue
        (ra, aa), (rb, ab) = fa[name], fb[name]
        aa = [] if aa is None else aa   # the parent left the argument-less getters untyped: ctypes then takes any call
        if ra is not rb:
            other.append(f"{name}: restype {describe(ra)} -> {describe(rb)}")
        if len(aa) != len(ab):
            other.append(f"{name}: {len(aa)} -> {len(ab)} arguments")
        for i, (a, b) in enumerate(zip(aa, ab)):
            if a is not b and describe(a) != describe(b):
                (expected if (name, i) in EXPECTED and b is ctypes.c_void_p else other).append(
                    f"{name} argument {i}: {describe(a)} -> {describe(b)}")
    sa, sb = structs_of(old), structs_of(new)
    for name in sorted(set(sa) | set(sb)):
        if name not in sa or name not in sb or layout(sa[name]) != layout(sb[name]):
            other.append(f"struct {name}: {layout(sa[name]) if name in sa else None} -> {layout(sb[name]) if name in sb else None}")
    ca = {k: v for k, v in vars(old).items() if k.isupper() and isinstance(v, int)}
    for name, v in sorted(ca.items()):
        if getattr(new, name, None) != v or type(getattr(new, name)) is not int:
            other.append(f"constant {name}: {v} -> {getattr(new, name, None)}")
    res = {"what": f"scorp_amd/_C.py as derived from include/scorp_gs.h against the hand-written tables of {parent}: restype and "
                   "argument classes of every function as lib() sets them on a recording stand-in for ctypes.CDLL, names, classes, "
                   "offsets and size of every struct, name and value of every constant the parent held",
           "parent": subprocess.check_output(["git", "-C", ROOT, "rev-parse", parent]).decode().strip(),
           "functions": len(fb), "functions_parent": len(fa), "arguments": sum(len(a) for _, a in fb.values()),
           "structs": len(sb), "structs_parent": len(sa), "struct_fields": sum(len(s._fields_) for s in sb.values()),
           "constants": len(new.CONSTANTS), "constants_parent": len(ca),
           "constants_new": sorted(set(new.CONSTANTS) - set(ca)),
           "untyped_in_parent": sorted(k for k, (_, a) in fa.items() if a is None),   # (void) getters: argtypes None there, [] here
           "differences_expected": expected, "differences_other": other,
           "import_seconds_median": {k: round(v, 4) for k, v in seconds.items()},
           "import_seconds_what": "one fresh interpreter per run, the module file executed alone (ctypes, os and, for the derived "
                                  "one, re included); median of 7, `import torch` median of 3"}
    with open(out_path, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(f"{len(fb)} functions, {len(sb)} structs, {len(new.CONSTANTS)} constants; {len(expected)} expected differences, "
          f"{len(other)} other; import {seconds}")
    for d in other:
        print("  " + d)
    return 1 if other or len(expected) != len(EXPECTED) else 0


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    sys.exit(main(*sys.argv[1:]))
