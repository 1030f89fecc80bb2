"""The C ABI read from include/fsg_hip.h: its `#define FSG_*` constants, its `typedef struct`s as ctypes.Structure classes and
its prototypes as ctypes (argtypes, restype).  The header is the one place where an entry point, a struct layout or a limit is
written; a declaration this reader does not understand is an error, never a guess."""
import ast
import ctypes
import operator
import re

SCALARS = {"int": ctypes.c_int, "int32_t": ctypes.c_int32, "int64_t": ctypes.c_int64, "long": ctypes.c_long,
           "size_t": ctypes.c_size_t, "float": ctypes.c_float, "double": ctypes.c_double}
HANDLES = ("fsg_stream_t",)   # typedefs of a pointer
RETURNS = dict(SCALARS, **{"const char *": ctypes.c_char_p, "void": None})
OPERATORS = {ast.LShift: operator.lshift, ast.BitOr: operator.or_, ast.Add: operator.add, ast.Sub: operator.sub,
             ast.Mult: operator.mul}


def _constant(name, text, defines):
    """value of `#define name text`: integer or float literals, << | + - *, parentheses and earlier defines -- nothing else"""
    def walk(node):
        if isinstance(node, ast.Constant) and type(node.value) in (int, float):
            return node.value
        if isinstance(node, ast.Name) and node.id in defines:
            return defines[node.id]
        if isinstance(node, ast.BinOp) and type(node.op) in OPERATORS:
            return OPERATORS[type(node.op)](walk(node.left), walk(node.right))
        raise ValueError(f"#define {name} {text}: not a constant expression over earlier FSG_ defines")
    literals = re.sub(r"\b(0[xX][0-9a-fA-F]+|\d+)[uUlL]*\b", r"\1", re.sub(r"\b(\d+\.\d*)[fF]\b", r"\1", text))   # C suffixes
    try:
        return walk(ast.parse(literals, mode="eval").body)
    except SyntaxError:
        raise ValueError(f"#define {name} {text}: not a constant expression over earlier FSG_ defines") from None


def _scalar(ctype_name, where):
    if ctype_name not in SCALARS:
        raise ValueError(f"{where}: unknown type '{ctype_name}'")
    return SCALARS[ctype_name]


def _fields(struct, body, defines):
    """`const float *a, *b; int n[FSG_MAX];` -> [("a", c_void_p), ("b", c_void_p), ("n", c_int * FSG_MAX)]"""
    fields = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        m = re.fullmatch(r"(?:const\s+)?(\w+)\s*(.*)", decl, re.S)
        for declarator in m.group(2).split(","):
            d = re.fullmatch(r"\s*(\*?)\s*(\w+)\s*(?:\[\s*(\w+)\s*\])?\s*", declarator)
            if not d:
                raise ValueError(f"struct {struct}: cannot read the declaration '{decl}'")
            star, field, dim = d.groups()
            ctype = ctypes.c_void_p if star or m.group(1) in HANDLES else _scalar(m.group(1), f"struct {struct}, field {field}")
            if dim is not None:
                if not dim.isdigit() and dim not in defines:
                    raise ValueError(f"struct {struct}, field {field}: array size '{dim}' is not defined")
                ctype = ctype * (int(dim) if dim.isdigit() else defines[dim])
            fields.append((field, ctype))
    return fields


def _argtype(function, arg):
    """a pointer of any kind (`*`, `[]`, a handle) is c_void_p -- callers pass data_ptr() or ctypes.byref; a scalar is its ctype"""
    words = re.sub(r"\bconst\b", " ", arg).split()
    if "*" in arg or "[" in arg or words[0] in HANDLES:
        return ctypes.c_void_p
    return _scalar(" ".join(words[:-1] or words), f"{function}, argument '{arg.strip()}'")


def parse(text):
    """header text -> (defines {name: value}, structs {name: ctypes.Structure class}, signatures {name: ([argtypes], restype)})"""
    text = re.sub(r"/\*.*?\*/|//[^\n]*", " ", text, flags=re.S)
    defines, structs, signatures = {}, {}, {}
    for name, value in re.findall(r"^[ \t]*#[ \t]*define[ \t]+(FSG_\w+)[ \t]+(\S[^\n]*)$", text, re.M):
        defines[name] = _constant(name, value.strip(), defines)
    for body, name in re.findall(r"^typedef\s+struct\s+\w*\s*\{(.*?)\}\s*(\w+)\s*;", text, re.M | re.S):
        structs[name] = type(name, (ctypes.Structure,), {"_fields_": _fields(name, body, defines)})
    for ret, name, args in re.findall(r"^([A-Za-z_][\w \t\*]*?)\s*\b(fsg_\w+)\s*\(([^)]*)\)\s*;", text, re.M):
        ret = " ".join(ret.replace("*", " * ").split())
        if ret not in RETURNS:
            raise ValueError(f"{name}: unknown return type '{ret}'")
        args = [] if args.strip() in ("", "void") else [_argtype(name, a) for a in args.split(",")]
        signatures[name] = (args, RETURNS[ret])
    return defines, structs, signatures


def load(path):
    try:
        with open(path) as f:
            return parse(f.read())
    except OSError as e:
        raise ImportError(f"{path}: the C header the ctypes binding is derived from cannot be read ({e})") from None
