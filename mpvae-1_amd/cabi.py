"""Reader of the project's C ABI headers (include/mpvae_hip.h, mpvae_host.h):
their constants, structs and prototypes as ctypes objects, so the Python
binding restates nothing.  A reader for these two headers, not a C front end:
no preprocessor, no compiler, and it never guesses -- whatever inside a struct
or at file scope it cannot match in full raises HeaderError with the text.

Type rules:
  scalar                 SCALARS below
  T name[N]              T * N, N an integer or a #define of the header
  struct by value        the parsed class
  pointer, struct field  c_void_p
  pointer, argument      POINTER(Struct) to a parsed struct, c_char_p for
                         const char*, c_void_p otherwise
  return                 a scalar, void, or const char* (c_char_p)
"""
import collections
import ctypes
import re

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64,
           "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "float": ctypes.c_float,
           "double": ctypes.c_double, "size_t": ctypes.c_size_t}
POINTEES = set(SCALARS) | {"void", "char", "uint8_t", "uint16_t"}  # behind a '*' only

Header = collections.namedtuple("Header", "constants structs prototypes")


class HeaderError(ValueError):
    """A declaration the reader does not fully understand."""


_INT = r"-?(?:0[xX][0-9a-fA-F]+|\d+)"
_DEFINE = re.compile(rf"#\s*define\s+(\w+)\s+({_INT})\s*$")  # MPV_LIVE(slot), guards: no match
_ITEM = re.compile(r"\s*(?:typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*(\w+)\s*;"
                   r"|enum\s+\w+\s*\{([^{}]*)\}\s*;|struct\s+(\w+)\s*;|([^;{}]+);)")
_ENUMERATOR = re.compile(rf"(\w+)(?:\s*=\s*({_INT}))?$")
_DECL = r"(const\s+)?(?:struct\s+)?(\w+)\s*(\*?)\s*"
_NAME = r"\w+(?:\s*\[\s*\w+\s*\])?"
_FIELD = re.compile(rf"{_DECL}({_NAME}(?:\s*,\s*{_NAME})*)$")
_PARAM = re.compile(rf"{_DECL}(\w+)$")
_PROTO = re.compile(rf"{_DECL}(\w+)\s*\(([^()]*)\)$")


def parse(path, known=None):
    """Header(constants, structs, prototypes) of the header at `path`.  `known`:
    structs of a header this one includes ({C name: class})."""
    def bad(what, text):
        raise HeaderError(f"{path}: {what}: {' '.join(text.split())!r}")

    text = re.sub(r"/\*.*?\*/", " ", open(path).read(), flags=re.S)
    text = re.sub(r"#\s*ifdef\s+__cplusplus\b.*?#\s*endif", " ", text, flags=re.S)  # extern "C"
    constants, structs, prototypes, declared = {}, {}, {}, set()
    named = dict(known or {})  # every struct in scope: `known` and, as they come, this header's

    def pointee(base, text):
        if base not in POINTEES and base not in named and base not in declared:
            bad("unknown pointee type", text)

    def struct(name, body, alias):
        if alias != name:
            bad("typedef name differs from the struct tag", f"{name} / {alias}")
        fields = []
        for decl in filter(None, (d.strip() for d in body.split(";"))):
            m = _FIELD.match(decl) or bad("unreadable struct member", decl)
            const, base, star, names = m.groups()
            names = [n.strip() for n in names.split(",")]
            if star and len(names) > 1:
                bad("several declarators behind one '*'", decl)
            if star:
                pointee(base, decl)
            t = ctypes.c_void_p if star else \
                SCALARS.get(base) or named.get(base) or bad("unknown base type", decl)
            for n in names:
                n, _, bound = n.rstrip("]").partition("[")
                if bound:
                    bound = bound.strip()
                    count = int(bound, 0) if re.fullmatch(_INT, bound) else constants.get(bound)
                    if count is None or count <= 0:
                        bad("array bound is not a known constant", decl)
                fields.append((n.strip(), t * count if bound else t))
        structs[name] = named[name] = type(name, (ctypes.Structure,), {"_fields_": fields})

    def prototype(text):
        m = _PROTO.match(text) or bad("unreadable declaration", text)
        const, base, star, name, params = m.groups()
        if star:
            res = ctypes.c_char_p if const and base == "char" else bad("pointer return", text)
        else:
            res = None if base == "void" else SCALARS.get(base) or bad("unknown return type", text)
        args = []
        for p in ([] if params.strip() == "void" else params.split(",")):
            pm = _PARAM.match(p.strip()) or bad("unreadable parameter", text)
            pconst, pbase, pstar, _ = pm.groups()
            if not pstar:
                args.append(SCALARS.get(pbase) or bad("unknown parameter type", text))
            elif pbase in named:
                args.append(ctypes.POINTER(named[pbase]))
            else:
                pointee(pbase, text)
                args.append(ctypes.c_char_p if pconst and pbase == "char" else ctypes.c_void_p)
        prototypes[name] = (res, args)

    lines = []
    for line in text.splitlines():
        if line.lstrip().startswith("#"):
            if not re.match(r"\s*#\s*(include|ifndef|define|endif)\b", line):
                bad("unsupported directive", line)  # #if, #pragma pack: could change a layout
            m = _DEFINE.match(line.strip())
            if m:
                constants[m.group(1)] = int(m.group(2), 0)
            line = ""
        lines.append(line)
    text, pos = "\n".join(lines), 0
    while text[pos:].strip():
        m = _ITEM.match(text, pos) or bad("unreadable declaration", text[pos:pos + 120])
        tag, body, alias, enum, forward, other = m.groups()
        if tag:
            struct(tag, body, alias)
        elif enum is not None:
            nxt = 0
            for e in filter(None, (e.strip() for e in enum.split(","))):
                em = _ENUMERATOR.match(e) or bad("unreadable enumerator", e)
                nxt = int(em.group(2), 0) if em.group(2) else nxt
                constants[em.group(1)], nxt = nxt, nxt + 1
        elif forward:
            declared.add(forward)
        else:
            prototype(other.strip())
        pos = m.end()
    return Header(constants, structs, prototypes)
