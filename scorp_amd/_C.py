"""ctypes binding of libscorp_gs.so, derived from include/scorp_gs.h: the header is the only description of the C ABI.

At import the header is read once and every prototype, `typedef struct` and `#define SCORP_<NAME> <literal>` in it becomes
FUNCTIONS[name] = (restype, argtypes), a ctypes.Structure under the header's name, and the constant <NAME>; lib() applies
the function table to the loaded library.  Adding an entry point means the header and its .hip definition, nothing here.

The reader (parse_header) is no C parser.  It accepts the style the header is written in and refuses everything else:
  - comments are /* ... */; the only directives are #include, the include guard, `#ifdef __cplusplus ... #endif` (its body
    is ignored) and `#define SCORP_<NAME> <literal>`, the literal an integer (`4`, `4u`), a parenthesised negative `(-4)` or
    a float `0.3f`; a #define without a value is a guard and gives no constant;
  - one declaration per `;`: `typedef void *<handle>;`, `typedef struct X { ... } X;` or a prototype
    `<scalar | const char *> name(<parameters | void>);`
  - scalars by their exact spelling: int, int32_t, uint32_t, int64_t, uint64_t, size_t, float, double.  A parameter or
    field is `[const] T name`, `[const] T *name` (T a scalar, void, uint8_t or an earlier struct of the header) or a
    handle; fields may also be arrays `T name[k]`, `T *name[k]` and share a line: `const float *x, *y, *z;`
  - no function pointers, no unions, no bit-fields, no nested structs by value, no macros in declarations.
Data pointers and handles travel as c_void_p (an integer, None, byref(...) or a ctypes array); a struct pointer PARAMETER
is POINTER(that struct), so a wrong struct is refused.  Anything else raises HeaderError naming the header line: there is
no fallback to int and no silent skip.

There is no CPU or PyTorch fallback: if the HIP library is missing or fails to load, importing the rasterizer raises.
Build it with `python -m scorp_amd.build` (or __graft_entry__.build()).
"""
import ctypes
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("SCORP_GS_LIB", os.path.join(_HERE, "libscorp_gs.so"))   # override: A/B builds of the library
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "scorp_gs.h")

_SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "uint32_t": ctypes.c_uint32, "int64_t": ctypes.c_int64,
            "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
_POINTEES = set(_SCALARS) | {"void", "uint8_t"}   # what a data pointer may point to, besides the header's own structs
_FIELD_RENAMES = {"in": "inputs"}                 # C field names that Python cannot spell
_DIRECTIVE = re.compile(r"#\s*(\w+)\s*(\w*)\s*(.*)")
_LITERAL = re.compile(r"(\d+)u?|\((-\d+)\)|(\d+\.\d+)f")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{")
_HANDLE = re.compile(r"typedef\s+void\s*\*\s*(\w+)")
_PROTOTYPE = re.compile(r"(const\s+char\s*\*|\w+)\s*\b(\w+)\s*\((.*)\)", re.S)
_DECLARATION = re.compile(r"(?:const\s+)?(\w+)\b\s*(.*)", re.S)
_DECLARATOR = re.compile(r"(\*?)\s*(\w+)\s*(?:\[\s*(\d+)\s*\])?")


class HeaderError(ValueError):
    pass


def parse_header(text):
    """(functions, structs, constants) of a header in the style of the module docstring: {name: (restype, argtypes)},
    {name: ctypes.Structure subclass} and {NAME without SCORP_: int or float}, each in the header's order."""
    functions, structs, constants, handles = {}, {}, {}, set()
    text = re.sub(r"/\*.*?\*/", lambda m: "\n" * m.group().count("\n"), text, flags=re.S)   # line numbers survive

    def fail(pos, why):
        raise HeaderError(f"scorp_gs.h line {text.count(chr(10), 0, pos) + 1}: {why}")

    def declare(pos, end, in_struct):
        """[(name, ctype)] of the declaration `[const] T declarator {, declarator}` at text[pos:end]"""
        pos += len(text[pos:end]) - len(text[pos:end].lstrip())
        decl = " ".join(text[pos:end].split())
        m = _DECLARATION.fullmatch(decl) or fail(pos, f"cannot read '{decl}'")
        base, out = m.group(1), []
        for d in m.group(2).split(","):
            m = _DECLARATOR.fullmatch(d.strip()) or fail(pos, f"cannot split the declarator '{d.strip()}' of '{decl}'")
            star, name, count = m.groups()
            if base not in _POINTEES and base not in structs and base not in handles:
                fail(pos, f"unknown type '{base}' in '{decl}'")
            if star and base not in handles:
                ctype = ctypes.c_void_p if in_struct or base not in structs else ctypes.POINTER(structs[base])
            elif not star and (base in _SCALARS or base in handles):
                ctype = _SCALARS.get(base, ctypes.c_void_p)
            else:
                fail(pos, f"'{base}' cannot be declared as '{d.strip()}' in '{decl}'")
            if count is not None:
                ctype = ctype * int(count) if in_struct else fail(pos, f"array parameter in '{decl}'")
            out.append((name, ctype))
        return out

    # the directives: constants out of the #defines, the body of `#ifdef __cplusplus` dropped, every directive blanked
    lines, offset, in_cplusplus = text.split("\n"), 0, False
    for i, line in enumerate(lines):
        m = _DIRECTIVE.fullmatch(line.strip())
        if m:
            kind, name, value = m.groups()
            if kind == "define" and name.startswith("SCORP_") and value:
                v = _LITERAL.fullmatch(value) or fail(offset, f"the value '{value}' of {name} is not a literal")
                constants[name[len("SCORP_"):]] = float(v.group(3)) if v.group(3) else int(v.group(1) or v.group(2))
            elif kind == "ifdef" and name == "__cplusplus":
                in_cplusplus = True
            elif kind == "endif":
                in_cplusplus = False
            elif not (kind == "define" and not value or kind == "ifndef" or kind == "include"):
                fail(offset, f"directive '{line.strip()}' is outside the accepted style")
        elif line.lstrip().startswith("#"):
            fail(offset, f"cannot read the directive '{line.strip()}'")
        offset += len(line) + 1
        if m or in_cplusplus:
            lines[i] = ""
    text = "\n".join(lines)

    pos = 0
    while True:
        pos += len(text[pos:]) - len(text[pos:].lstrip())
        if pos == len(text):
            return functions, structs, constants
        struct = _STRUCT.match(text, pos)
        if struct:
            name = struct.group(1)
            closing = re.compile(r"\}\s*%s\s*;" % name).search(text, struct.end())
            if not closing:
                fail(pos, f"struct {name} is not closed by '}} {name};'")
            fields, at = [], struct.end()
            while ";" in text[at:closing.start()]:
                semi = text.index(";", at)
                fields += [(_FIELD_RENAMES.get(n, n), t) for n, t in declare(at, semi, True)]
                at = semi + 1
            if text[at:closing.start()].strip():
                fail(at, f"'{text[at:closing.start()].strip()}' in struct {name} does not end in ';'")
            structs[name] = type(name, (ctypes.Structure,), {"_fields_": fields})
            pos = closing.end()
            continue
        end = text.find(";", pos)
        stmt = " ".join(text[pos:end if end >= 0 else len(text)].split())
        handle, proto = _HANDLE.fullmatch(stmt), _PROTOTYPE.fullmatch(stmt)
        if end < 0:
            fail(pos, f"'{stmt}' does not end in ';'")
        elif handle:
            handles.add(handle.group(1))
        elif proto and proto.group(1) != "typedef":
            ret, name, params = proto.groups()
            restype = _SCALARS.get(ret) or (ctypes.c_char_p if "*" in ret else fail(pos, f"unknown return type '{ret}' of {name}"))
            args, at = [], text.index("(", pos) + 1
            for p in ([] if params.strip() == "void" else text[at:text.rindex(")", at, end)].split(",")):
                args += [t for _, t in declare(at, at + len(p), False)]
                at += len(p) + 1
            functions[name] = (restype, args)
        else:
            fail(pos, f"cannot read '{stmt}'")
        pos = end + 1


with open(HEADER_PATH) as _f:
    FUNCTIONS, STRUCTS, CONSTANTS = parse_header(_f.read())
EXPORTS = list(FUNCTIONS)
globals().update(STRUCTS)      # _C.ScorpGs3dInputs, ...
globals().update(CONSTANTS)    # _C.ERR_INVALID, _C.BACKWARD_EXACT_FP32, ...

_lib = None


def lib():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise RuntimeError(
            f"{LIB_PATH} not found: the HIP extension is not built. Run `python -m scorp_amd.build` "
            "(needs /opt/rocm/bin/hipcc). scorp_amd has no CPU fallback.")
    # PyTorch-ROCm bundles its own libamdhip64; it must be the HIP runtime already in the process when this library
    # is loaded, or the kernels register with a second runtime that has no device ("no ROCm-capable device").
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    for name, (restype, argtypes) in FUNCTIONS.items():
        if not hasattr(L, name):
            raise RuntimeError(f"{LIB_PATH} does not export {name}, which include/scorp_gs.h declares: the library is stale, "
                               "rebuild it with `python -m scorp_amd.build`.")
        fn = getattr(L, name)
        fn.restype, fn.argtypes = restype, argtypes
    _lib = L
    return L


def current_stream_ptr():
    """The current HIP stream of the current device as an integer.  torch.cuda.current_stream() builds a Stream object through
    three layers of device-index helpers (9 us a call, six calls per training iteration); the raw getter is 0.3 us."""
    import torch
    try:
        return int(torch._C._cuda_getCurrentRawStream(torch._C._cuda_getDevice()))
    except AttributeError:   # (a torch build without the raw getters)
        return int(torch.cuda.current_stream().cuda_stream)


def prof_enable(on=True, only=None):
    """Start / stop hipEvent bracketing of the library's kernels; `only` = iterable of kernel names to bracket."""
    L = lib()
    mask = (1 << 64) - 1
    if only is not None:
        names = [L.scorp_prof_kernel_name(k).decode() for k in range(L.scorp_prof_num_kernels())]
        mask = sum(1 << names.index(n) for n in only)
    check(L.scorp_prof_select(mask), "scorp_prof_select")
    check(L.scorp_prof_enable(1 if on else 0), "scorp_prof_enable")


def prof_collect():
    """{kernel name: (total ms, launches)} of the kernels timed since prof_enable(True); synchronises."""
    L = lib()
    n = L.scorp_prof_num_kernels()
    ms = (ctypes.c_double * n)()
    cnt = (ctypes.c_uint64 * n)()
    check(L.scorp_prof_collect(ms, cnt), "scorp_prof_collect")
    return {L.scorp_prof_kernel_name(k).decode(): (ms[k], int(cnt[k])) for k in range(n)}


def check(code, what):
    if code != 0:
        msg = lib().scorp_last_error()
        raise RuntimeError(f"{what} failed ({code}): {msg.decode(errors='replace') if msg else ''}")


def call(name, *args):
    """lib().<name>(*args, current stream), checked under its name: a tensor goes as its data_ptr(), a ctypes.Structure by
    reference, None and everything else as given.  For the callers that are not per-iteration hot paths (scorp_amd/mesh)."""
    import torch
    check(getattr(lib(), name)(*[a.data_ptr() if isinstance(a, torch.Tensor) else ctypes.byref(a) if isinstance(a, ctypes.Structure) else a
                                 for a in args], current_stream_ptr()), name)


def call_with_workspace(name, size_name, size_args, *args):
    """call(name, *args, workspace, size) for the entry points that take a one-call workspace as their last two arguments:
    size = lib().<size_name>(*size_args) bytes, allocated as a uint8 tensor on the device of the first tensor of args, under
    that device's guard."""
    import torch
    dev = next(a.device for a in args if isinstance(a, torch.Tensor))
    with torch.cuda.device(dev):
        size = getattr(lib(), size_name)(*size_args)
        workspace = torch.empty(size, dtype=torch.uint8, device=dev)
        call(name, *args, workspace, size)
