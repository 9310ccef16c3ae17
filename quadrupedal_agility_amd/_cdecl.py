"""Reader of the C declarations of include/*.h: the one place the ABI is written down.  _capi.py builds its ctypes layer from what this finds:

    consts       {name: value} of every `#define NAME <number or expression of earlier names>` and every enumerator, in declaration order
    struct(name) the ctypes.Structure generated from `typedef struct [tag] { ... } name;`
    prototypes   [(header, name, restype, argtypes)] of every `ret qa_<name>(args);`

The dialect is what the headers use, read with regular expressions after the comments are gone; there is no preprocessor (`#if` lines are dropped
unevaluated: the headers have only include guards and the `extern "C"` guard).  Nothing is skipped: text that none of the patterns consumes, a field
or parameter of an unknown type, or a `qa_name(` that did not become a prototype raises a ValueError naming the header and the declaration."""
import ctypes as C
import os
import re

INCLUDE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include")
SCALARS = {"int": C.c_int32, "int32_t": C.c_int32, "int64_t": C.c_int64, "uint32_t": C.c_uint32, "uint64_t": C.c_uint64,
           "float": C.c_float, "double": C.c_double}

consts, structs, prototypes = {}, {}, []


def _value(header, expr):
    """a constant expression: numbers (`1u`, `0.5f`, `(-1)`), names read earlier, and + - * | between them"""
    py = re.sub(r"\b(\d+)[uU]\b", r"\1", re.sub(r"\b(\d+\.\d*|\.\d+)f\b", r"\1", expr))
    if not re.fullmatch(r"[\w\s.()|+*-]+", py):
        raise ValueError(f"{header}: not a constant expression: `{expr}`")
    try:
        return eval(py, {"__builtins__": {}}, consts)
    except Exception as e:
        raise ValueError(f"{header}: cannot evaluate `{expr}`: {e}") from None


def _enum(header, body):
    nxt = 0
    for item in filter(None, (s.strip() for s in body.split(","))):
        name, _, expr = (s.strip() for s in item.partition("="))
        consts[name] = nxt = _value(header, expr) if expr else nxt
        nxt += 1


def _struct(header, name, body):
    fields = []
    for decl in filter(None, (s.strip() for s in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s+(.+)", decl, re.S)            # `const float *a, *b`, `float kp, kd`, `int32_t ids[QA_N][2]`
        base, declarators = (m.group(1), m.group(2).split(",")) if m else (None, [""])
        for d in declarators:
            dm = re.fullmatch(r"\s*(\**)\s*(\w+)\s*((?:\[[^\]]+\]\s*)*)", d)
            ctype = None if not dm else C.c_void_p if dm.group(1) else SCALARS.get(base) or structs.get(base)
            if ctype is None:
                raise ValueError(f"{header}: struct {name}: cannot read `{decl}`")
            for dim in reversed(re.findall(r"\[([^\]]+)\]", dm.group(3))):   # a[2][3] is two of three: the last dimension is the innermost type
                ctype = ctype * _value(header, dim)
            fields.append((dm.group(2), ctype))
    structs[name] = type("".join(p.capitalize() for p in name.split("_")), (C.Structure,),
                         {"_fields_": fields, "__doc__": f"{name} of include/{header}"})


def _prototype(header, ret, name, params):
    ret, argtypes = " ".join(ret.split()), []
    restype = C.c_char_p if ret == "const char *" else SCALARS.get(ret)
    if restype is None:
        raise ValueError(f"{header}: {name}: unknown return type `{ret}`")
    for p in [] if params.strip() == "void" else params.split(","):
        m = re.fullmatch(r"\s*(?:const\s+)?(\w+)\s+\w+\s*", p)                # a pointer or array parameter has a * or [ and is an address
        if "*" not in p and "[" not in p and not (m and m.group(1) in SCALARS):
            raise ValueError(f"{header}: {name}: cannot read parameter `{p.strip()}`")
        argtypes.append(SCALARS[m.group(1)] if m else C.c_void_p)
    prototypes.append((header, name[len("qa_"):], restype, argtypes))


def _read(header):
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", open(os.path.join(INCLUDE, header)).read(), flags=re.S)
    calls = len(re.findall(r"qa_[a-z0-9_]+\s*\(", text))
    before = len(prototypes)

    def take(pattern, fn, flags=0):
        nonlocal text
        text = re.sub(pattern, lambda m: fn(header, *m.groups()) or " ", text, flags=flags)

    take(r"^[ \t]*#[ \t]*define[ \t]+(\w+)[ \t]+(\S.*)$", lambda h, name, expr: consts.__setitem__(name, _value(h, expr)), re.M)
    take(r"^[ \t]*#.*$", lambda h: None, re.M)                                   # include guards, #include, #ifdef __cplusplus
    take(r'extern\s+"C"\s*\{', lambda h: None)
    take(r"\benum\s*\w*\s*\{([^}]*)\}\s*;", _enum)
    take(r"\btypedef\s+struct\s*\w*\s*\{([^}]*)\}\s*(\w+)\s*;", lambda h, body, name: _struct(h, name, body))
    take(r"\btypedef\s+struct\s+(\w+)\s+\1\s*;", lambda h, tag: None)            # an opaque handle: only ever behind a pointer
    take(r"([\w\s*]+?)\b(qa_\w+)\s*\(([^()]*)\)\s*;", _prototype)
    if text.strip() != "}" or len(prototypes) - before != calls:                # "}" closes extern "C"
        raise ValueError(f"include/{header}: {calls} `qa_name(` but {len(prototypes) - before} prototypes read; text not understood: `{text.strip()[:200]}`")


def struct(name):
    return structs[name]


def values(prefix, names):
    """consts[prefix + n] for the space-separated names"""
    return tuple(consts[prefix + n] for n in names.split())


def names(prefix):
    """the constants called <prefix>*, which must count 0, 1, 2, ... in declaration order, without the prefix: the order an enum states"""
    found = [n for n in consts if n.startswith(prefix)]
    if [consts[n] for n in found] != list(range(len(found))):
        raise ValueError(f"{prefix}* do not count from 0 in declaration order")
    return [n[len(prefix):] for n in found]


for _h in ["qa_sim.h"] + sorted(f for f in os.listdir(INCLUDE) if f.endswith(".h") and f != "qa_sim.h"):   # the others use its constants and structs
    _read(_h)
