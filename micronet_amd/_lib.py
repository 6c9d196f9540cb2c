"""ctypes binding of ``libmicronet_hip.so`` (C ABI declared in ``include/micronet_hip.h``).

The product path has NO fallback: if the gfx950 library is missing, or it is the CPU emulation build the unit
tests use, ``get_lib()`` raises.  Every entry point returns 0 or a negative errno-style code; ``check`` turns a
failure into a Python exception carrying ``mn_last_error()``.
"""
import ctypes as C
import os
import re

HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("MN_LIB_PATH") or os.path.join(HERE, "lib", "libmicronet_hip.so")   # MN_LIB_PATH: ablation builds of the same library
HEADER_PATH = os.path.join(HERE, "..", "include", "micronet_hip.h")


class MicronetHipError(RuntimeError):
    pass


class ConvGeom(C.Structure):
    pass


class ActQ(C.Structure):
    pass


class WQ(C.Structure):
    """mn_wq: how the fake-quantised fp32 weights factor into integer codes x per-channel scale."""


class ProfEntry(C.Structure):
    pass


class AdamTensor(C.Structure):
    pass


class I8ResAdd(C.Structure):
    """mn_i8res_add: the quantizers of the add stage of the int8 ResNet deployment."""


class I8FirstOuts(C.Structure):
    """mn_i8first_outs: the output quantizers of the two-output first block of the int8 ResNet deployment."""


class I8ZQuant(C.Structure):
    """mn_i8z_quant: one quantizer (scale, zero point, asymmetric flag, bits) of the int8 deployment with zero points."""


# C struct name -> class: the one thing stated here and not read from the header (the classes get their _fields_ below)
STRUCTS = {"mn_conv_geom": ConvGeom, "mn_actq": ActQ, "mn_wq": WQ, "mn_prof_entry": ProfEntry, "mn_adam_tensor": AdamTensor, "mn_i8res_add": I8ResAdd,
           "mn_i8z_quant": I8ZQuant, "mn_i8first_outs": I8FirstOuts}

_SCALARS = {"int": C.c_int, "int32_t": C.c_int32, "int64_t": C.c_int64, "float": C.c_float, "double": C.c_double}
_RETURNS = dict(_SCALARS, **{"void": None, "const char*": C.c_char_p})
_DEFINE = re.compile(r"#\s*define\s+(MN_\w+)\b(.*)")
_INTEGER = re.compile(r"\(\s*(-?\d+)\s*\)|(0[xX][0-9a-fA-F]+|0|[1-9]\d*)")
_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;")
_FIELD = re.compile(r"(?:const\s+)?(\w*)(.*)", re.S)
_DECLARATOR = re.compile(r"(\*[\s*]*)?(\w+)\s*(?:\[\s*(\d+)\s*\])?")
_FUNCTION = re.compile(r"(.*?)\b(\w+)\s*\(([^()]*)\)")
_PARAM = re.compile(r"(?:const\s+)?(\w+)\s*((?:\*\s*(?:const\s*)?)*)(\w+)?")


def parse_header(text):
    """``(constants, struct_fields, prototypes)`` of a header written in the vocabulary of ``include/micronet_hip.h``: integer ``#define MN_*``, ``typedef void* T;``,
    ``typedef struct X { ... } X;`` for the names in ``STRUCTS``, and function declarations over int / int32_t / int64_t / float / double, those structs and pointers.
    Anything else raises ``MicronetHipError`` naming the item: a construct this reader does not know must fail the import, never be skipped or taken for an int."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    constants, lines = {}, []
    for line in text.split("\n"):
        if not line.lstrip().startswith("#"):
            lines.append(line)
            continue
        m = _DEFINE.match(line.strip())
        if m:
            v = _INTEGER.fullmatch(m.group(2).strip())
            if not v:
                raise MicronetHipError("header: #define %s is not an integer constant: %r" % (m.group(1), m.group(2).strip()))
            constants[m.group(1)] = int(v.group(1) or v.group(2), 0)
    text = "\n".join(lines)

    aliases = set(re.findall(r"typedef\s+void\s*\*\s*(\w+)\s*;", text))             # mn_stream_t
    text = re.sub(r"typedef\s+void\s*\*\s*\w+\s*;", " ", text)

    struct_fields = {}
    for tag, body, name in _STRUCT.findall(text):
        if tag != name or name not in STRUCTS or name in struct_fields:
            raise MicronetHipError("header: struct %s { ... } %s: not one of _lib.STRUCTS, or declared twice" % (tag, name))
        fields = struct_fields[name] = []
        for stmt in filter(None, (s.strip() for s in body.split(";"))):
            base, rest = _FIELD.fullmatch(stmt).groups()
            for decl in rest.split(","):
                d = _DECLARATOR.fullmatch(decl.strip())
                if not d:
                    raise MicronetHipError("header: struct %s: cannot read field %r" % (name, stmt))
                stars, field, dim = d.groups()
                if stars and not dim:
                    ctype = C.c_void_p
                elif base == "char" and dim and not stars:
                    ctype = C.c_char * int(dim)
                elif base in _SCALARS and not dim:
                    ctype = _SCALARS[base]
                else:
                    raise MicronetHipError("header: struct %s: field %s has a type outside the vocabulary: %r" % (name, field, stmt))
                fields.append((field, ctype))
    text = _STRUCT.sub(" ", text)

    text, opened = re.subn(r'extern\s+"C"\s*\{', " ", text)
    prototypes, closed = {}, 0
    for stmt in text.split(";"):
        stmt = " ".join(stmt.split())
        while stmt.startswith("}"):
            closed, stmt = closed + 1, stmt[1:].strip()
        if not stmt:
            continue
        m = _FUNCTION.fullmatch(stmt)
        if not m:
            raise MicronetHipError("header: not a declaration this reader knows: %r" % stmt)
        ret, name, params = m.group(1), m.group(2), m.group(3).strip()
        ret = re.sub(r"\s*\*\s*", "*", ret.strip())
        if name in prototypes:
            raise MicronetHipError("header: %s is declared twice" % name)
        if ret not in _RETURNS:
            raise MicronetHipError("header: %s: return type outside the vocabulary: %r" % (name, ret))
        argtypes = []
        for param in ([] if params in ("", "void") else params.split(",")):
            p = _PARAM.fullmatch(param.strip())
            base, stars = (p.group(1), p.group(2).count("*")) if p else (None, 0)
            if stars == 1 and base in STRUCTS:
                argtypes.append(C.POINTER(STRUCTS[base]))
            elif stars or base in aliases:
                argtypes.append(C.c_void_p)
            elif base in _SCALARS:
                argtypes.append(_SCALARS[base])
            else:
                raise MicronetHipError("header: %s: parameter type outside the vocabulary: %r" % (name, param.strip()))
        prototypes[name] = (_RETURNS[ret], argtypes)
    if opened != closed:
        raise MicronetHipError('header: unbalanced extern "C" braces (%d opened, %d closed)' % (opened, closed))
    return constants, struct_fields, prototypes


def _read_header():
    try:
        with open(HEADER_PATH) as f:
            return parse_header(f.read())
    except OSError as e:
        raise MicronetHipError("cannot read the C ABI header %s: %s" % (HEADER_PATH, e))


# every integer #define MN_* of the header becomes a module attribute; PROTOTYPES: name -> (restype, argtypes) of every function the header declares
_CONSTANTS, _FIELDS, PROTOTYPES = _read_header()
globals().update(_CONSTANTS)
for _name, _cls in STRUCTS.items():
    _cls._fields_ = _FIELDS[_name]


class Lib:
    def __init__(self, path):
        self.path = path
        self.cdll = C.CDLL(path)
        for name, (res, args) in PROTOTYPES.items():
            fn = getattr(self.cdll, name)      # AttributeError if the symbol is not exported
            fn.restype = res
            fn.argtypes = args
            setattr(self, name, fn)

    def check(self, rc, what=""):
        if rc != 0:
            msg = self.mn_last_error()
            raise MicronetHipError("%s failed (rc=%d): %s" % (what, rc, msg.decode() if msg else ""))
        return rc


_LIB = None


def load(path):
    return Lib(path)


def get_lib():
    """The gfx950 library, or an exception -- never a CPU fallback."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise MicronetHipError(
                "libmicronet_hip.so not built (%s). Run `python -c 'import __graft_entry__ as g; g.build()'` "
                "or `python -m micronet_amd.build`; there is no CPU fallback." % LIB_PATH)
        lib = Lib(LIB_PATH)
        if lib.mn_is_emulation():
            raise MicronetHipError("%s is an emulation build; the product requires the gfx950 build" % LIB_PATH)
        _LIB = lib
    return _LIB
