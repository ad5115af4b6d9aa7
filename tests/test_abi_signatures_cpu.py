"""arx/_lib.py PROTOTYPES against include/arx.h by TYPE: return type, number of parameters, every by-value parameter
exactly, every pointer parameter against a pointer type of the right pointee.  (The export test of test_oracle_cpu.py
compares the names only; an i32 written for an i64 in a 30-argument list corrupts a call silently.)

Needs no built library and never imports arx: the header is parsed as text, and of arx/_lib.py only the part up to
the end of PROTOTYPES is executed (the ctypes aliases and the table), without its `import torch`."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

N_ENTRY_POINTS = 146

# C scalar -> ctypes.  (ctypes aliases types of equal layout -- c_int is c_int32, c_size_t is c_uint64 on LP64 --, so
# the comparison is by class identity: what the call passes, not how it was spelled.)
SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "size_t": C.c_size_t,
           "uint64_t": C.c_uint64, "uint8_t": C.c_uint8, "uint16_t": C.c_uint16, "uint32_t": C.c_uint32,
           "char": C.c_char}
RETURNS = {("int", 0): C.c_int, ("size_t", 0): C.c_size_t, ("char", 1): C.c_char_p}


def parse_header(text):
    """{name: (ret, [param, ...])} with ret / param = (base type without const, number of '*')."""
    text = re.sub(r"/\*.*?\*/", " ", text, flags=re.S)
    text = re.sub(r"//[^\n]*", " ", text)
    text = "\n".join(l for l in text.split("\n") if not l.lstrip().startswith("#"))   # (a #define above a declaration
    text = text.replace('extern "C" {', " ")                                          #  would leak into its return type)

    def ctype(s, named):
        stars = s.count("*")
        words = [w for w in s.replace("*", " ").split() if w != "const"]
        if named and len(words) > 1:
            words = words[:-1]                   # the parameter's name
        assert len(words) == 1, s
        return words[0], stars
    decls = {}
    for stmt in text.split(";"):
        m = re.match(r"^\s*(?:\}\s*)?(.*?)\b(arx_[a-z0-9_]+)\s*\((.*)\)\s*$", stmt, flags=re.S)
        if not m:
            assert "arx_" not in stmt or "(" not in stmt, "unparsed declaration: %r" % stmt
            continue
        ret, name, params = m.group(1), m.group(2), " ".join(m.group(3).split())
        assert name not in decls, name
        plist = [] if params in ("", "void") else [ctype(p, True) for p in params.split(",")]
        decls[name] = (ctype(ret, False), plist)
    return decls


def load_prototypes():
    lines = open(os.path.join(ROOT, "a-recsys_amd", "arx", "_lib.py")).read().split("\n")
    end = next(i for i, l in enumerate(lines) if l.startswith("class ArxError"))
    src = "\n".join(l for l in lines[:end] if not l.startswith("import torch"))
    assert "PROTOTYPES = {" in src
    ns = {"__file__": "_lib.py"}
    exec(compile(src, "_lib.py(prototypes)", "exec"), ns)
    return ns["PROTOTYPES"]


def _is_pointer(t):
    return isinstance(t, type) and issubclass(t, C._Pointer)


def mismatches(name, decl, proto):
    """The disagreements between one parsed declaration and one PROTOTYPES entry, as strings (none: [])."""
    (rbase, rstars), params = decl
    res, args = proto
    out = []
    if RETURNS.get((rbase, rstars)) is not res:
        out.append("%s: returns %s%s, bound as %s" % (name, rbase, "*" * rstars, getattr(res, "__name__", res)))
    if len(params) != len(args):
        out.append("%s: %d parameters, %d bound" % (name, len(params), len(args)))
        return out
    for k, ((base, stars), a) in enumerate(zip(params, args)):
        what = "%s: parameter %d (%s%s) bound as %s" % (name, k, base, "*" * stars, getattr(a, "__name__", a))
        if stars == 0:
            ok = SCALARS.get(base) is a
        elif a is C.c_void_p:
            ok = True                             # device pointers travel as integers
        elif _is_pointer(a):
            ok = a._type_ is (C.c_void_p if stars > 1 else SCALARS.get(base))
        else:
            ok = a is C.c_char_p and base == "char" and stars == 1        # a host string buffer (arx_device_info)
        if not ok:
            out.append(what)
    return out


def test_prototypes_match_arx_h_by_type():
    decls = parse_header(open(os.path.join(ROOT, "include", "arx.h")).read())
    protos = load_prototypes()
    assert len(decls) == N_ENTRY_POINTS, len(decls)
    assert len(protos) == N_ENTRY_POINTS, len(protos)
    assert sorted(decls) == sorted(protos)
    bad = [m for name in sorted(decls) for m in mismatches(name, decls[name], protos[name])]
    assert not bad, "\n".join(bad)


def test_comparator_reports_corrupted_entries():
    """Not vacuous: three corrupted copies of one real entry are each reported."""
    name = "arx_sparse_adagrad_cat_multi"
    decl = parse_header(open(os.path.join(ROOT, "include", "arx.h")).read())[name]
    res, args = load_prototypes()[name]
    assert mismatches(name, decl, (res, args)) == []
    k64 = next(k for k, a in enumerate(args) if a is C.c_int64)
    narrowed = list(args)
    narrowed[k64] = C.c_int32                                     # one i64 replaced by i32
    assert any("parameter %d " % k64 in m for m in mismatches(name, decl, (res, narrowed)))
    dropped = list(args)
    del dropped[k64]                                              # one argument dropped
    assert any("bound" in m and "parameters" in m for m in mismatches(name, decl, (res, dropped)))
    kp = next(k for k, a in enumerate(args) if _is_pointer(a) and a._type_ is C.c_int64)
    repointed = list(args)
    repointed[kp] = C.POINTER(C.c_int32)                          # POINTER(i64) replaced by POINTER(i32)
    assert any("parameter %d " % kp in m for m in mismatches(name, decl, (res, repointed)))
