"""ctypes loader for libmusicxl.so (the C-ABI boundary, include/musicxl.h).

There is NO fallback: if the library is missing or a call returns non-zero, we raise.  A product path that silently
ran on PyTorch/CPU would void every parity claim.
"""
import ctypes as C
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('MXL_LIB_PATH') or os.path.join(_HERE, 'libmusicxl.so')   # override: A/B builds of the library
HEADER_PATH = os.path.join(_HERE, '..', 'include', 'musicxl.h')

_lib = None


class MusicXLError(RuntimeError):
    pass


_CTYPE = {
    'int': C.c_int, 'unsigned': C.c_uint, 'float': C.c_float, 'unsigned long long': C.c_ulonglong,
    'long long': C.c_longlong, 'size_t': C.c_size_t,
}


def declared_functions(header_path: str = HEADER_PATH):
    """Parse `include/musicxl.h` -> {name: (restype, [argtypes])}.  The header is the single source of truth."""
    src = open(header_path).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for m in re.finditer(r'(const char\*|int|size_t)\s+(mxl_\w+)\s*\(([^;{]*?)\)\s*;', src, flags=re.S):
        ret, name, args = m.group(1), m.group(2), m.group(3).strip()
        argtypes = []
        if args and args != 'void':
            for a in args.split(','):
                a = ' '.join(a.split())
                if '*' in a:
                    argtypes.append(C.c_void_p)
                else:
                    ty = ' '.join(a.split(' ')[:-1])
                    ty = ty.replace('const ', '')
                    argtypes.append(_CTYPE[ty])
        restype = C.c_char_p if ret.startswith('const char') else (C.c_size_t if ret == 'size_t' else C.c_int)
        out[name] = (restype, argtypes)
    return out


def declared_structs(header_path: str = HEADER_PATH):
    """Parse the `typedef struct mxl_x { ... } mxl_x;` blocks of `include/musicxl.h` -> {name: ctypes.Structure class}: a field
    with a `*` is a c_void_p, a scalar goes through _CTYPE, and one line may declare several fields (`int eos_id, pad_id;`)."""
    src = open(header_path).read()
    src = re.sub(r'/\*.*?\*/', '', src, flags=re.S)
    out = {}
    for m in re.finditer(r'typedef\s+struct\s+(mxl_\w+)\s*\{(.*?)\}\s*\1\s*;', src, flags=re.S):
        fields = []
        for decl in m.group(2).split(';'):
            decl = ' '.join(decl.split())
            if not decl:
                continue
            first, *more = [d.strip() for d in decl.split(',')]
            ty, name = first.rsplit(' ', 1)                    # `const unsigned char* cls` / `int eos_id`: the type, the first name
            ctype = C.c_void_p if '*' in first else _CTYPE[ty.replace('const ', '')]
            if '*' in first and more:
                raise MusicXLError(f'{m.group(1)}: one pointer field per declaration ({decl!r})')
            fields += [(n.lstrip('*'), ctype) for n in [name] + more]
        out[m.group(1)] = type(m.group(1), (C.Structure,), {'_fields_': fields})
    return out


_structs = None


def struct(name: str):
    """the ctypes class of a struct the header declares (parsed once)"""
    global _structs
    if _structs is None:
        _structs = declared_structs()
    return _structs[name]


def lib():
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise MusicXLError(
                f'{LIB_PATH} not found: build it with `python __graft_entry__.py` (hipcc, gfx950). '
                'There is no CPU / PyTorch fallback for the product path.')
        # torch first: it ships its own libamdhip64, and the library must bind to THAT copy of the HIP runtime -- loaded before torch it
        # pulls in /opt/rocm's, the process then holds two runtimes, and every call through the second one fails with
        # hipErrorNoDevice (seen with __graft_entry__.build() followed by smoke() in one process)
        import torch  # noqa: F401
        _lib = C.CDLL(LIB_PATH)
        for name, (restype, argtypes) in declared_functions().items():
            fn = getattr(_lib, name)  # AttributeError if the header declares something the .so lacks
            fn.restype = restype
            fn.argtypes = argtypes
        if _lib.mxl_abi_version() != 3:
            raise MusicXLError('libmusicxl ABI version mismatch')
        if C.sizeof(struct('mxl_rules')) != _lib.mxl_rules_size():
            raise MusicXLError(f'mxl_rules is {C.sizeof(struct("mxl_rules"))} bytes as parsed from the header, '
                               f'{_lib.mxl_rules_size()} in the library')
    return _lib


def check(code: int, what: str = ''):
    if code != 0:
        msg = lib().mxl_error_string(code)
        raise MusicXLError(f'{what} failed with code {code}: {msg.decode() if msg else "?"}')
