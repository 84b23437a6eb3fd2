"""What include/sp_hip.h declares, read with regular expressions: the prototypes by type class, the integer ``#define SP_*`` values and
the ``typedef struct`` records laid out by natural alignment -- what tests/test_abi_mirror.py holds super_primitive_amd/_lib.py to.

No C front end: the header is regular (one declaration per ``;``, no bit fields, no unions, no nested braces), and whatever falls
outside that raises ``ValueError`` here instead of being guessed at."""
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "sp_hip.h")

POINTER = "pointer"
# what a ctypes argument list can say about a non-pointer parameter or return value
ARG_CLASSES = ("int", "long long", "float", "double")
# bytes of the scalar field types, each aligned to its own size
SCALARS = {"int8_t": 1, "uint8_t": 1, "char": 1, "int16_t": 2, "uint16_t": 2, "int32_t": 4, "uint32_t": 4, "int": 4, "float": 4,
           "int64_t": 8, "uint64_t": 8, "long long": 8, "double": 8}
POINTER_BYTES = 8

_INT_TOKEN = re.compile(r"\s*(?:(0[xX][0-9a-fA-F]+|\d+)(?:[uU]?[lL]{0,2})\b|([A-Za-z_]\w*)|(<<|>>|[()|&^~+\-*]))")


def strip_comments(text):
    return re.sub(r"/\*.*?\*/", " ", text, flags=re.S)


def int_expr(expr, defines):
    """The value of an integer constant expression over literals, earlier defines and ( ) | & ^ ~ + - * << >>; None when it is not one."""
    pos, out = 0, []
    expr = expr.strip()
    while pos < len(expr):
        m = _INT_TOKEN.match(expr, pos)
        if not m:
            return None
        lit, name, op = m.groups()
        if name is not None and name not in defines:
            return None
        out.append(str(int(lit, 0)) if lit is not None else str(defines[name]) if name is not None else op)
        pos = m.end()
    try:
        return int(eval(" ".join(out), {"__builtins__": {}})) if out else None
    except SyntaxError:
        return None


def type_class(text, what):
    """'pointer', 'int', 'long long', 'float' or 'double' of a parameter or return type (qualifiers dropped); anything else raises."""
    if "*" in text:
        return POINTER
    words = " ".join(w for w in text.split() if w != "const")
    if words not in ARG_CLASSES:
        raise ValueError(f"{what}: type {text.strip()!r} is none of pointer, {', '.join(ARG_CLASSES)}")
    return words


def parse_defines(text):
    """{name: value} of every object-like ``#define SP_*`` whose value is an integer expression."""
    defines = {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(SP_\w+)[ \t]+(\S.*)$", text, flags=re.M):
        val = int_expr(value, defines)
        if val is not None:
            defines[name] = val
    return defines


def _layout(name, body, defines, structs):
    fields, offset, align = [], 0, 1
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        first, *rest = [d.strip() for d in decl.split(",")]
        m = re.fullmatch(r"(.*?[\s*])(\w+)\s*((?:\[[^\]]*\]\s*)*)", first, flags=re.S)
        if not m:
            raise ValueError(f"struct {name}: cannot read the declaration {decl!r}")
        base = " ".join(w for w in m.group(1).replace("*", " ").split() if w not in ("const", "struct"))
        declarators = [("*" in m.group(1), m.group(2), m.group(3))]
        for d in rest:
            r = re.fullmatch(r"(\**)\s*(\w+)\s*((?:\[[^\]]*\]\s*)*)", d)
            if not r:
                raise ValueError(f"struct {name}: cannot read the declarator {d!r} of {decl!r}")
            declarators.append((bool(r.group(1)), r.group(2), r.group(3)))
        for is_ptr, field, dims in declarators:
            if is_ptr:
                size = al = POINTER_BYTES
            elif base in SCALARS:
                size = al = SCALARS[base]
            elif base in structs:
                size, al = structs[base]["size"], structs[base]["align"]
            else:
                raise ValueError(f"struct {name}: field {field} has the unknown type {base!r}")
            for dim in re.findall(r"\[([^\]]*)\]", dims):
                n = int_expr(dim, defines)
                if n is None or n <= 0:
                    raise ValueError(f"struct {name}: field {field} has the dimension {dim!r}")
                size *= n
            offset = -(-offset // al) * al
            fields.append((field, offset, size))
            offset += size
            align = max(align, al)
    if not fields:
        raise ValueError(f"struct {name}: no fields")
    return {"fields": fields, "size": -(-offset // align) * align, "align": align, "stated": None}


def parse(path=HEADER):
    """(prototypes, defines, structs) of the header:
    prototypes  {name: (return class, [argument class, ...], [argument name, ...])}
    defines     {name: int}
    structs     {name: {"fields": [(name, offset, size), ...], "size", "align", "stated": the SP_ABI_SIZE number or None}}"""
    with open(path) as f:
        text = strip_comments(f.read())
    defines = parse_defines(text)
    text = re.sub(r"^[ \t]*#(?:.*\\\n)*.*$", " ", text, flags=re.M)            # preprocessor lines, continued ones included
    text = re.sub(r'extern\s+"C"\s*\{', " ", text)

    structs = {}

    def take_struct(m):
        tag, body, name = m.groups()
        if "{" in body or (tag and tag != name) or name in structs:
            raise ValueError(f"struct {name}: nested braces, a tag that differs from the name, or a second definition")
        structs[name] = _layout(name, body, defines, structs)
        return " "
    text = re.sub(r"typedef\s+struct\s*(\w*)\s*\{(.*?)\}\s*(\w+)\s*;", take_struct, text, flags=re.S)

    def take_size(m):
        name, n = m.group(1), int(m.group(2))
        if name not in structs or structs[name]["stated"] is not None:
            raise ValueError(f"SP_ABI_SIZE({name}, {n}): no such struct above it, or stated twice")
        structs[name]["stated"] = n
        return " "
    text = re.sub(r"\bSP_ABI_SIZE\s*\(\s*(\w+)\s*,\s*(\d+)\s*\)", take_size, text)
    text = re.sub(r"\bSP_ABI_ASSERT\s*\([^;]*?\"[^\"]*\"\s*\)", " ", text)

    prototypes = {}
    for stmt in filter(None, (s.strip() for s in text.split(";"))):
        if stmt == "}" or re.fullmatch(r"struct\s+\w+", stmt):                  # the end of extern "C", a forward declaration
            continue
        m = re.fullmatch(r"(.*?[\s*])(\w+)\s*\((.*)\)", stmt, flags=re.S)
        if not m or m.group(2) in prototypes:
            raise ValueError(f"cannot read the declaration {stmt!r}")
        name, args = m.group(2), m.group(3).strip()
        arg_classes, arg_names = [], []
        if args not in ("", "void"):
            for i, arg in enumerate(args.split(",")):
                a = re.fullmatch(r"(.*?[\s*])(\w+)", arg.strip(), flags=re.S)      # every parameter is named
                if not a:
                    raise ValueError(f"{name}: cannot read parameter {i}, {arg.strip()!r}")
                arg_classes.append(type_class(a.group(1), f"{name}, parameter {a.group(2)}"))
                arg_names.append(a.group(2))
        prototypes[name] = (type_class(m.group(1), f"{name}, return value"), arg_classes, arg_names)
    return prototypes, defines, structs
