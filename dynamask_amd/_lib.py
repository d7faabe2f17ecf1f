"""ctypes loader of libdynamask_hip.so (the C ABI of include/dynamask_hip.h)."""
import ctypes
import functools
import os

from . import _abi, hazard
from ._abi import DynaMaskLibraryError  # noqa: F401  (raised here and by the header parse)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get('DYNAMASK_HIP_LIB') or os.path.join(_HERE, 'libdynamask_hip.so')      # override: kernel experiments
REQUIRED_BUILD_FLAG = '-packed-fp32-ops'        # dynamask_amd/build.py NO_PACKED_FP32; dm_build_info() must carry it

_vp = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def _derived():
    """What this module takes from include/dynamask_hip.h (_abi.py).  Computed at first use: the parse takes longer
    than importing ctypes does, so it is not paid at import."""
    protos, consts = _abi.load()

    class PackJob(ctypes.Structure):
        """dm_pack_job of include/dynamask_hip.h (hand-written; tests/test_abi_cpu.py compares the layout)."""
        _fields_ = [('w', _vp), ('w_packed', _vp), ('Cout', ctypes.c_int), ('Cin', ctypes.c_int), ('ksize', ctypes.c_int),
                    ('transpose_flip', ctypes.c_int), ('num_srcs', ctypes.c_int),
                    ('src_channels', ctypes.c_int * consts['DM_MAX_SOURCES']), ('ld', ctypes.c_int), ('c0', ctypes.c_int)]

    return {'SIGNATURES': {n: ([t for t, _ in args], res) for n, (res, args) in protos.items()},  # name -> (argtypes, restype)
            'ABI_VERSION': consts['DM_ABI_VERSION'], 'PackJob': PackJob}


def __getattr__(name):          # _lib.SIGNATURES, _lib.ABI_VERSION, _lib.PackJob
    if name in ('SIGNATURES', 'ABI_VERSION', 'PackJob'):
        return _derived()[name]
    raise AttributeError(f'module {__name__!r} has no attribute {name!r}')


_LIB = None
_PROXY = None       # hazard.wrap_lib(_LIB), handed out while the stream-hazard tracker is on (DM_HAZARD, hazard.ENABLED)


def check_build_info(info):
    """Refuse a library that does not say it was compiled without packed fp32 (include/dynamask_hip.h dm_build_info)."""
    if REQUIRED_BUILD_FLAG not in info and os.environ.get('DM_ALLOW_PACKED_FP32') != '1':
        raise DynaMaskLibraryError(
            f'{LIB_PATH} was not built with {REQUIRED_BUILD_FLAG!r} (dm_build_info: {info!r}): packed fp32 '
            'instructions dropped a product under multi-queue load (profiles/r05_race_hunt.txt).  Rebuild with '
            '`python -m dynamask_amd.build`, or set DM_ALLOW_PACKED_FP32=1 for an A/B measurement')


def lib():
    """Load the library once.  Fails loudly: there is no fallback path."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIB_PATH):
            raise DynaMaskLibraryError(
                f'{LIB_PATH} not found: build it with `python -m dynamask_amd.build` '
                '(or __graft_entry__.build()); dynamask_amd has no CPU/eager fallback')
        # PyTorch-ROCm ships its own libamdhip64; import it FIRST so that the
        # process has exactly one HIP runtime (the library's DT_NEEDED
        # libamdhip64.so.7 then binds to the copy torch already loaded, and the
        # streams / device pointers torch hands us belong to the same runtime).
        import torch  # noqa: F401
        L = ctypes.CDLL(LIB_PATH)
        for name, (argtypes, restype) in _derived()['SIGNATURES'].items():
            try:
                fn = getattr(L, name)
            except AttributeError:
                # (entry points that are only added keep ABI_VERSION: a library from before them has the number right
                # and lacks the symbol)
                raise DynaMaskLibraryError(f'libdynamask_hip.so lacks {name}: it is older than this package, '
                                           'rebuild') from None
            fn.argtypes = argtypes
            fn.restype = restype
        if L.dm_abi_version() != _derived()['ABI_VERSION']:
            raise DynaMaskLibraryError('libdynamask_hip.so ABI version mismatch: rebuild')
        check_build_info(L.dm_build_info().decode())
        _LIB = L
    if hazard.ENABLED[0]:
        global _PROXY
        if _PROXY is None:
            _PROXY = hazard.wrap_lib(_LIB)
        return _PROXY
    return _LIB


def check(rc, what):
    if rc != 0:
        msg = lib().dm_error_string(rc).decode()
        raise RuntimeError(f'{what} failed: {msg} (code {rc})')
