"""The C ABI as include/dynamask_hip.h declares it: the one parse behind _lib.SIGNATURES and hazard.parse_header()."""
import ctypes
import os
import re

HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'include', 'dynamask_hip.h')

_SCALARS = {'int': ctypes.c_int, 'float': ctypes.c_float, 'double': ctypes.c_double, 'long long': ctypes.c_longlong}
_RESTYPES = {'int': ctypes.c_int, 'long long': ctypes.c_longlong, 'const char*': ctypes.c_char_p}
_POINTEES = set(_SCALARS) | {'void', 'char', 'int32_t', 'int64_t', 'uint8_t', 'unsigned long long', 'dm_pack_job'}
_PROTO = re.compile(r'([^;{}]*?)\b(dm_[a-z0-9_]+)\s*\(([^;{}]*)\)\s*;')
_ARG = re.compile(r'(const )?((?:unsigned )?long long|\w+) ?(\* ?const ?\*|\*)? ?\w*')


class DynaMaskLibraryError(RuntimeError):
    pass


def _arg(a, decl):
    """One parameter -> (ctypes type, hazard role: 'in' (const T*), 'out' (T*), 'in[]' / 'out[]' (host array of device
    pointers), 'stream', 'scalar')."""
    m = _ARG.fullmatch(a)
    const, base, stars = m.groups() if m else (None, None, None)
    if base == 'dm_stream_t' and not const and not stars:
        return ctypes.c_void_p, 'stream'
    if not stars and not const and base in _SCALARS:
        return _SCALARS[base], 'scalar'
    if stars and base in _POINTEES:
        role = ('in' if const else 'out') + ('[]' if len(stars) > 1 else '')
        return (ctypes.c_char_p if base == 'char' and stars == '*' else ctypes.c_void_p), role
    raise DynaMaskLibraryError(f'dynamask_hip.h: cannot marshal parameter {a!r} of `{decl}`')


def parse(text):
    """(prototypes, constants) of a header text: {name: (restype, [(ctype, role), ...])} for every dm_* prototype and
    {name: int} for every integer ``#define DM_*``.  Strict: a declaration it cannot marshal raises, none is skipped."""
    text = re.sub(r'/\*.*?\*/', '', text, flags=re.S)
    constants = {k: int(v) for k, v in re.findall(r'^[ \t]*#[ \t]*define[ \t]+(DM_\w+)[ \t]+\(?(-?\d+)\)?[ \t]*$', text, flags=re.M)}
    text = re.sub(r'^[ \t]*#.*$', '', text, flags=re.M)
    protos = {}
    for ret, name, args in _PROTO.findall(text):
        ret, args = ' '.join(ret.split()), ' '.join(args.split())
        decl = f'{ret} {name}({args});'
        if ret not in _RESTYPES:
            raise DynaMaskLibraryError(f'dynamask_hip.h: return type of `{decl}` is none of {sorted(_RESTYPES)}')
        protos[name] = (_RESTYPES[ret], [] if args in ('void', '') else [_arg(a.strip(), decl) for a in args.split(',')])
    skipped = set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', text)) - set(protos)
    if skipped:
        raise DynaMaskLibraryError(f'dynamask_hip.h: {sorted(skipped)} not understood as prototypes')
    return protos, constants


_LOADED = {}


def load(path=HEADER):
    """parse() of the header file, read once per process."""
    if path not in _LOADED:
        try:
            with open(path) as f:
                text = f.read()
        except OSError as e:
            raise DynaMaskLibraryError(f'{path}: the C header the bindings are derived from cannot be read ({e})') from None
        _LOADED[path] = parse(text)
    return _LOADED[path]
