"""Parser of include/unet_hip.h: the header is the one description of the C ABI and `_lib`
derives the ctypes binding from what `parse` returns.  Pure text processing (no torch, no library).

The parser fails loudly: a directive, declaration or type outside the small C subset the header
is written in raises `HeaderError` naming it; nothing is skipped.
"""
import collections
import functools
import re

SCALARS = ("int", "float", "double", "size_t", "int64_t", "uint64_t")
_POINTEES = SCALARS + ("void", "char", "uint8_t", "uint16_t", "uint32_t")
_MARKS = ("UNET_HOST", "UNET_DEVICE")     # the header's empty macros: where a pointer lives

# version: UNET_ABI_VERSION; structs: name -> [(C type, field)]; functions: name -> (return C type,
# [(C type, parameter)]), all in the header's order
Header = collections.namedtuple("Header", "version structs functions")


_STRUCT = re.compile(r"typedef\s+struct\s+(\w+)\s*\{([^{}]*)\}\s*\1\s*;")
_FUNCTION = re.compile(r"([^()]*[\w*])\s*\b(unet_\w+)\s*\(([^()]*)\)")
_DIRECTIVE = re.compile(
    r"\s*#\s*(?:(?:ifndef|ifdef|endif|include)\b.*|define\s+(\w+)\s*(.*?))\s*")
_SPACE = re.compile(r"\s*")


class HeaderError(ValueError):
    pass


@functools.lru_cache(maxsize=None)    # a header has some twenty distinct types in 1800 places
def classify(ctype, structs, is_return=False):
    """The class of a C type of the header: a name of SCALARS; "void*" (unet_stream_t, every
    device or untyped pointer, a `unet_X* UNET_DEVICE` table in device memory); "char*" (a returned
    string); ("host", scalar) for a `scalar* UNET_HOST` the host dereferences; ("struct", name)
    for a pointer to a record of the header in host memory.  structs: the frozenset of the
    header's struct names."""
    tokens = [t for t in ctype.replace("*", " * ").split() if t != "const"]
    marks = [t for t in tokens if t in _MARKS]
    tokens = [t for t in tokens if t not in _MARKS]
    stars = tokens.count("*")
    if not tokens or len(marks) > 1 or tokens[1:] != ["*"] * stars or stars > 1 or \
            (marks and not stars):
        raise HeaderError(f"cannot classify the type '{ctype}'")
    base = tokens[0]
    if base.startswith("unet_") and stars:
        if base not in structs:
            raise HeaderError(f"'{ctype}' names a struct the header does not define")
        if marks != ["UNET_HOST"]:
            return "void*" if marks else ("struct", base)
    elif marks:
        if marks == ["UNET_HOST"] and base in SCALARS:
            return ("host", base)
    elif not stars:
        if base in SCALARS:
            return base
        if base == "unet_stream_t":
            return "void*"
    elif base == "char" and is_return:
        return "char*"
    elif base in _POINTEES:
        return "void*"
    raise HeaderError(f"cannot classify the type '{ctype}'")


def _declarator(text, where):
    """'const float* UNET_HOST mean3' -> ('const float* UNET_HOST', 'mean3')"""
    *ctype, name = text.replace("*", "* ").split() or [""]
    if not ctype or not name.isidentifier():
        raise HeaderError(f"cannot split '{text.strip()}' into a type and a name in {where}")
    return " ".join(ctype).replace(" *", "*"), name


def _fields(body, name):
    fields = []
    for line in filter(None, (s.strip() for s in body.split(";"))):
        first, *more = line.split(",")     # `int Cout, Cin;`
        ctype, field = _declarator(first, name)
        if (more and "*" in ctype) or not all(re.fullmatch(r"\s*\w+\s*", m) for m in more):
            raise HeaderError(f"cannot read the declarators of '{line}' in {name}")
        fields += [(ctype, f.strip()) for f in [field] + more]
    return fields


def parse(text):
    """Header text -> Header.  Raises HeaderError on anything it cannot classify."""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    version, code = None, []
    for line in text.splitlines():
        if not line.lstrip().startswith("#"):
            code.append(line)
            continue
        m = _DIRECTIVE.fullmatch(line)
        if not m or line.rstrip().endswith("\\"):
            raise HeaderError(f"cannot read the directive '{line.strip()}'")
        if m.group(1) == "UNET_ABI_VERSION":
            version = int(m.group(2))
    if version is None:
        raise HeaderError("no #define UNET_ABI_VERSION")
    text, extern_c = re.subn(r'extern\s+"C"\s*\{', "", "\n".join(code))
    text = text.strip()
    structs, functions, pos = {}, {}, 0
    while pos < len(text):
        if extern_c and text[pos] == "}":
            extern_c, end = extern_c - 1, pos + 1
        elif m := _STRUCT.match(text, pos):
            structs[m.group(1)] = _fields(m.group(2), m.group(1))
            end = m.end()
        else:
            end = text.find(";", pos) + 1
            decl = " ".join(text[pos:end - 1 if end else pos + 80].split())
            if not end:
                raise HeaderError(f"unterminated declaration '{decl}'")
            m = _FUNCTION.fullmatch(decl)
            if m and m.group(2) not in functions:
                name, params = m.group(2), m.group(3).strip()
                functions[name] = (re.sub(r"\s*\*", "*", m.group(1)),
                                   [] if params == "void" else
                                   [_declarator(p, name) for p in params.split(",")])
            elif decl != "typedef void* unet_stream_t":
                raise HeaderError(f"cannot read the declaration '{decl}' (or it is a second one)")
        pos = _SPACE.match(text, end).end()

    names = frozenset(structs)

    def check(owner, ctype, is_return=False):
        try:
            return classify(ctype, names, is_return)
        except HeaderError as e:
            raise HeaderError(f"{owner}: {e}") from None
    for name, fields in structs.items():
        for ctype, field in fields:
            if isinstance(check(name, ctype), tuple):
                raise HeaderError(f"{name}.{field}: '{ctype}' is not a scalar or a plain pointer")
    for name, (ret, params) in functions.items():
        check(name, ret, is_return=True)
        for ctype, _ in params:
            check(name, ctype)
    return Header(version, structs, functions)
