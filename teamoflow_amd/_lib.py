"""ctypes binding of libtmf.so (C ABI in include/tmf.h).

The engine has no CPU implementation: every entry point needs the gfx950 code object and a
visible MI355X.  ``get()`` raises ``EngineUnavailable`` loudly instead of falling back to anything.

include/tmf.h is the only statement of the ABI: ``parse_header`` reads the constants, the structs and
the prototypes from it, and the ctypes structures and ``SIGNATURES`` are made from what it read.  An
entry point is added by declaring it in the header.  The grammar ``parse_header`` accepts, and refuses
to go beyond (``ValueError`` naming the declaration, never a default type):
  - comments, ``#ifdef __cplusplus .. #endif`` blocks and preprocessor lines other than ``#define`` are dropped;
  - ``#define TMF_NAME integer`` (the integer may stand in parentheses); a ``#define`` without a value is a guard;
  - ``typedef struct tag { fields } name;`` with fields ``type a, b;`` or ``const type* a;`` - no arrays,
    no nested structs;
  - ``type tmf_name(void);`` and ``type tmf_name(type a, const type* b, ...);`` - every parameter named,
    one declarator each, no arrays, no function pointers;
  - type = int, int32_t, int64_t, size_t, float, double or a struct by value; pointers to those, to
    uint16_t, void, a struct, and ``const char*``.
"""
import collections
import ctypes
import os
import re
import subprocess

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('TMF_LIB', os.path.join(_HERE, 'libtmf.so'))
CSRC = os.path.join(_HERE, 'csrc')
HEADER_PATH = os.path.join(_HERE, os.pardir, 'include', 'tmf.h')


class EngineUnavailable(RuntimeError):
    pass


class EngineError(RuntimeError):
    pass


# constants: NAME -> int; structs: typedef name -> [(C type, field)]; functions: name -> (C return type, [C parameter types])
Header = collections.namedtuple('Header', 'constants structs functions')
_DECLARATOR = re.compile(r'(const\s+)?(\w+)(\s*\*\s*|\s+)(\w+(?:\s*,\s*\w+)*)')


def _typed_names(decl, where):
    """'const int32_t* a' -> ('const int32_t*', ['a']); 'float a, b' -> ('float', ['a', 'b'])."""
    m = _DECLARATOR.fullmatch(decl.strip())
    if not m:
        raise ValueError(f'{where}: cannot read the declaration `{" ".join(decl.split())}`')
    const, base, star, names = m.groups()
    return ('const ' if const else '') + base + star.strip(), re.split(r'\s*,\s*', names)


def parse_header(text):
    text = re.sub(r'/\*.*?\*/|//[^\n]*', ' ', text, flags=re.S)
    text = re.sub(r'^[ \t]*#[ \t]*ifdef[ \t]+__cplusplus\b.*?^[ \t]*#[ \t]*endif\b', '', text, flags=re.S | re.M)
    constants, structs, functions = {}, {}, {}
    for name, value in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(TMF_\w+)[ \t]*(.*)$', text, re.M):
        value = value.strip()
        if value.startswith('(') and value.endswith(')'):
            value = value[1:-1]
        try:
            if value:
                constants[name] = int(value, 0)
        except ValueError:
            raise ValueError(f'#define {name}: `{value}` is not an integer') from None
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)

    def struct(m):
        tag, body, name = m.groups()
        if '{' in body:
            raise ValueError(f'struct {tag}: nested braces')
        structs[name] = [(ctype, field) for decl in body.split(';') if decl.strip()
                         for ctype, fields in [_typed_names(decl, 'struct ' + name)] for field in fields]
        return ''
    text = re.sub(r'\btypedef\s+struct\s+(\w+)\s*\{(.*?)\}\s*(\w+)\s*;', struct, text, flags=re.S)
    for decl in filter(str.strip, text.split(';')):
        m = re.fullmatch(r'([^()]+)\((.*)\)', decl.strip(), re.S)
        if not m:
            raise ValueError(f'cannot read the declaration `{" ".join(decl.split())}`')
        ret, (name,) = _typed_names(m.group(1), 'prototype')
        params = [] if m.group(2).strip() == 'void' else m.group(2).split(',')
        functions[name] = (ret, [_typed_names(p, name)[0] for p in params])
    return Header(constants, structs, functions)


_SCALARS = {'int': ctypes.c_int, 'int32_t': ctypes.c_int32, 'int64_t': ctypes.c_int64, 'size_t': ctypes.c_size_t,
            'float': ctypes.c_float, 'double': ctypes.c_double}
_POINTEE_BYTES = {'void': 0, 'uint16_t': 2, **{name: ctypes.sizeof(t) for name, t in _SCALARS.items()}}


class TensorPointer(ctypes.c_void_p):
    """The argtype of a data-pointer parameter: takes what c_void_p takes (None, an int, a c_void_p ..) and a torch.Tensor, whose
    elements must have the size of the header's pointee type (void: any).  Size, not dtype: the engine reinterprets on purpose in
    places.  No device and no contiguity check: plans are built on CPU tensors too, and views are legal arguments."""
    pointee, pointee_bytes = 'void', 0

    @classmethod
    def from_param(cls, obj):
        if isinstance(obj, torch.Tensor):
            if cls.pointee_bytes and obj.element_size() != cls.pointee_bytes:
                raise TypeError(f'a {obj.dtype} tensor ({obj.element_size()}-byte elements) for a `{cls.pointee}*` parameter')
            return ctypes.c_void_p(obj.data_ptr())
        return ctypes.c_void_p.from_param(obj)


_pointer_types = {'void': TensorPointer}


def tensor_pointer(pointee):
    """One TensorPointer class per pointee type, so that two prototypes with the same C types have equal argtypes."""
    if pointee not in _pointer_types:
        _pointer_types[pointee] = type(pointee + '_p', (TensorPointer,), {'pointee': pointee, 'pointee_bytes': _POINTEE_BYTES[pointee]})
    return _pointer_types[pointee]


def _ctype(ctype, structs, where, field=False):
    base = ctype.replace('const ', '').rstrip('*')
    if not ctype.endswith('*'):
        t = _SCALARS.get(base) or structs.get(base)
    elif base in structs:
        t = ctypes.POINTER(structs[base])
    elif base in _POINTEE_BYTES:           # a struct's pointers stay untyped: they are filled in from data_ptr() sums
        t = ctypes.c_void_p if field else tensor_pointer(base)
    else:
        t = ctypes.c_char_p if ctype == 'const char*' else None
    if t is None:
        raise ValueError(f'{where}: unknown type `{ctype}`')
    return t


def bind(header):
    """The ctypes side of a parsed header: ({typedef name: Structure class}, {name: (restype, argtypes)})."""
    structs = {}
    for name, fields in header.structs.items():
        fields = [(f, _ctype(t, structs, f'struct {name}', field=True)) for t, f in fields]
        structs[name] = type(name[4:].title().replace('_', ''), (ctypes.Structure,), {'_fields_': fields})   # tmf_slice_lists: SliceLists
    return structs, {name: (_ctype(ret, structs, name), [_ctype(t, structs, name) for t in args])
                     for name, (ret, args) in header.functions.items()}


with open(HEADER_PATH) as _fh:
    HEADER = parse_header(_fh.read())
_STRUCTS, SIGNATURES = bind(HEADER)   # SIGNATURES: name -> (restype, argtypes)
Adam, Segments, SliceLists, Exclusion, RankRows = (_STRUCTS[_n] for _n in ('tmf_adam', 'tmf_segments', 'tmf_slice_lists',
                                                                           'tmf_exclusion', 'tmf_rank_rows'))
_F, _P = ctypes.c_float, tensor_pointer('void')   # `float`, and `void*` (the stream, a workspace)
MIN_LIB_VERSION = HEADER.constants['TMF_VERSION']
EPI_ADAM, EPI_GRAD = HEADER.constants['TMF_EPI_ADAM'], HEADER.constants['TMF_EPI_GRAD']
SLICE_XCD_MAJOR, SLICE_N_ITEMS_STATED = HEADER.constants['TMF_SLICE_XCD_MAJOR'], HEADER.constants['TMF_SLICE_N_ITEMS_STATED']   # tmf_slice_lists.flags

_lib = None


def build(force=False, verbose=False):
    """Compile libtmf.so in-tree with hipcc for gfx950 (cross-compiles without a GPU)."""
    if force:
        subprocess.run(['make', '-C', CSRC, 'clean'], check=True, capture_output=not verbose)
    subprocess.run(['make', '-C', CSRC, '-j4'], check=True, capture_output=not verbose)
    return LIB_PATH


def load_library():
    """dlopen libtmf.so and attach the signatures.  Needs no GPU (used by the CPU symbol test).
    torch is imported first on purpose: its bundled libamdhip64 (SONAME libamdhip64.so.7) is then
    already in the process and libtmf's DT_NEEDED entry resolves to that same runtime, so torch's
    streams and allocations are valid inside the library."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise EngineUnavailable(f'{LIB_PATH} not found - run `python -c "import __graft_entry__ as g; g.build()"` '
                                f'or `make -C {CSRC}`')
    lib = ctypes.CDLL(LIB_PATH)
    older = os.environ.get('TMF_LIB_OLDER') == '1'   # A/B runs against a library built from an older commit (tools/c4_ab.sh)
    # the version first: a stale library then says so instead of failing on the first symbol it lacks
    try:
        lib.tmf_version.restype, lib.tmf_version.argtypes = SIGNATURES['tmf_version']
        version = lib.tmf_version()
    except AttributeError:
        version = 0
    if version < MIN_LIB_VERSION and not older:
        raise EngineUnavailable(f'{LIB_PATH} is version {version}, this package needs {MIN_LIB_VERSION} or newer (struct layouts and '
                                f'entry points changed) - rebuild it: `make -C {CSRC}`')
    for name, (res, args) in SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError:
            if older:
                continue
            raise EngineUnavailable(f'{LIB_PATH} (version {version}) lacks {name} - rebuild it: `make -C {CSRC}`') from None
        fn.restype, fn.argtypes = res, args
    _lib = lib
    return lib


def get():
    """The library, ready to launch on the current torch device.  Raises if there is no GPU."""
    if not torch.cuda.is_available():
        raise EngineUnavailable('teamoflow_amd needs an MI355X: torch.cuda.is_available() is False and the '
                                'engine has no CPU fallback')
    return load_library()


def stream_ptr():
    return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def ptr(t):
    if t is None:
        return None
    return ctypes.c_void_p(t.data_ptr())


def check(rc, lib=None):
    if rc != 0:
        lib = lib or load_library()
        raise EngineError(f'libtmf error {rc}: {lib.tmf_last_error().decode()}')


def padded_ld(n_components, dtype=None):
    """Mirror of tmf_padded_ld / tmf_padded_ld_bf16, usable without loading the library."""
    r = int(n_components)
    if r < 1 or r > 1024:
        raise ValueError(f'n_components={r} outside the supported range [1, 1024]')
    if dtype is torch.bfloat16:
        if r > 512:
            return 1024
        lanes, g = (r + 7) // 8, 1
        while g < lanes:
            g *= 2
        return 8 * g
    if r <= 256:
        lanes, g = (r + 3) // 4, 1
        while g < lanes:
            g *= 2
        return 4 * g
    nv = (r + 255) // 256
    if nv == 3:
        nv = 4
    return 256 * nv
