"""The ctypes bindings are derived from include/dynamask_hip.h (dynamask_amd/_abi.py): the parser on synthetic headers,
hand-written pins on the real one, the layout of the one hand-written structure, the one definition of the ABI number.
No GPU needed."""
import ctypes
import os
import re
import subprocess

import pytest

from dynamask_amd import _abi, _lib, hazard

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, 'include', 'dynamask_hip.h')
API_MISC = os.path.join(ROOT, 'dynamask_amd', 'csrc', 'api_misc.hip')

VP, CP, I, F, D, LL = ctypes.c_void_p, ctypes.c_char_p, ctypes.c_int, ctypes.c_float, ctypes.c_double, ctypes.c_longlong

SYNTHETIC = '''
#define DM_OK 0
#define DM_ERR_UNSUPPORTED (-3)   /* valid request */
#define DM_MAX_SOURCES 4
#define DM_NOT_A_NUMBER "x"
typedef void* dm_stream_t; /* hipStream_t */
typedef struct dm_pack_job { const float* w; int src_channels[DM_MAX_SOURCES]; } dm_pack_job;
int dm_pointers(const float* a, float* b, const float* const* c, float* const* d, const int* e, const long long* f,
                const dm_pack_job* g, char* h, dm_stream_t stream);
/* a comment that looks like a call: dm_fake(1, 2);
 * int dm_fake2(int); */
int dm_scalars(int a, float b, double c, long long d);
long long dm_nothing(void);
const char*
dm_three_lines(int code,
               float scale);
'''


def test_synthetic_header_gives_exact_types_and_roles():
    protos, consts = _abi.parse(SYNTHETIC)
    assert list(protos) == ['dm_pointers', 'dm_scalars', 'dm_nothing', 'dm_three_lines']
    assert protos['dm_pointers'] == (I, [(VP, 'in'), (VP, 'out'), (VP, 'in[]'), (VP, 'out[]'), (VP, 'in'), (VP, 'in'),
                                         (VP, 'in'), (CP, 'out'), (VP, 'stream')])
    assert protos['dm_scalars'] == (I, [(I, 'scalar'), (F, 'scalar'), (D, 'scalar'), (LL, 'scalar')])
    assert protos['dm_nothing'] == (LL, [])
    assert protos['dm_three_lines'] == (CP, [(I, 'scalar'), (F, 'scalar')])
    assert consts == {'DM_OK': 0, 'DM_ERR_UNSUPPORTED': -3, 'DM_MAX_SOURCES': 4}


@pytest.mark.parametrize('decl', ['unsigned dm_x(int);', 'int dm_x(size_t n);', 'void dm_x(void);', 'int dm_x(int (*cb)(int));',
                                  'int dm_x(const int n);', 'int dm_x(dm_stream_t* s);', 'int dm_x(int n) { return n; }',
                                  'static inline int dm_x(int n);'])
def test_parser_refuses_what_it_cannot_marshal(decl):
    with pytest.raises(_abi.DynaMaskLibraryError, match='dm_x'):
        _abi.parse('typedef void* dm_stream_t;\nint dm_ok(int n);\n' + decl + '\nint dm_after(void);\n')


def test_missing_header_raises_with_the_path(tmp_path):
    with pytest.raises(_lib.DynaMaskLibraryError, match='no_such_header.h'):
        _abi.load(str(tmp_path / 'no_such_header.h'))


def test_no_prototype_of_the_real_header_is_skipped():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r'\b(dm_[a-z0-9_]+)\s*\(', text))
    protos, consts = _abi.load()
    assert set(protos) == declared and len(protos) == len(_lib.SIGNATURES) >= 148
    assert _abi.load() is _abi.load(_abi.HEADER)                       # one parse per process
    assert hazard.parse_header() == {n: [r for _, r in args] for n, (_, args) in protos.items()}
    assert _lib.SIGNATURES == {n: ([t for t, _ in args], res) for n, (res, args) in protos.items()}
    assert consts['DM_OK'] == 0 and (consts['DM_ERR_INVALID_ARG'], consts['DM_ERR_LAUNCH'], consts['DM_ERR_UNSUPPORTED']) == (-1, -2, -3)
    assert consts['DM_MAX_LEVELS'] == 4 and consts['DM_MAX_SOURCES'] == 4 and consts['DM_AUG_VIEW_FLOATS'] == 8


def test_hand_written_pins_on_the_real_header():
    """Written from the header by hand, not through the parser: where a wrong scalar type would hand a kernel garbage."""
    S = _lib.SIGNATURES
    a, r = S['dm_random_sample']
    assert len(a) == 24 and a[12] is D and a[11] is I and a[13] is VP and r is I
    assert S['dm_rle_string'] == ([VP, I, LL, CP, LL], LL)
    a = S['dm_roi_align_fwd_ws'][0]
    assert a[15] is LL and a[14] is VP and a[16] is VP and a[11] is F and len(a) == 17
    assert S['dm_group_norm_supported'] == ([LL, I, I, I, I], I)
    a = S['dm_sigmoid_bwd'][0]
    assert [i for i, t in enumerate(a) if t is LL] == [1, 3, 5]
    a = S['dm_sgd_momentum_step'][0]
    assert [i for i, t in enumerate(a) if t is F] == [4, 5, 6, 7] and a[3] is LL and a[8] is I
    assert S['dm_error_string'] == ([I], CP) and S['dm_build_info'] == ([], CP)
    assert S['dm_abi_version'] == ([], I) and S['dm_roi_align_workspace_bytes'] == ([I, I], LL)


def test_pack_job_layout_matches_the_compiled_header(tmp_path):
    """The one hand-written ctypes.Structure against sizeof / offsetof as the compiler lays dm_pack_job out."""
    fields = [f for f, _ in _lib.PackJob._fields_]
    src = tmp_path / 'layout.cpp'
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "dynamask_hip.h"\nint main() {\n'
                   '  printf("sizeof %zu\\n", sizeof(dm_pack_job));\n'
                   + ''.join(f'  printf("{f} %zu\\n", offsetof(dm_pack_job, {f}));\n' for f in fields)
                   + '  printf("DM_MAX_SOURCES %d\\n", DM_MAX_SOURCES);\n  return 0;\n}\n')
    exe = tmp_path / 'layout'
    hipcc = os.environ.get('HIPCC', '/opt/rocm/bin/hipcc')                # what dynamask_amd/build.py compiles with
    subprocess.check_call([hipcc, '-x', 'c++', '-std=c++17', '-I' + os.path.join(ROOT, 'include'), str(src), '-o', str(exe)])
    out = dict(line.split() for line in subprocess.check_output([str(exe)], text=True).splitlines())
    assert set(out) == set(fields) | {'sizeof', 'DM_MAX_SOURCES'} and len(fields) == 10
    assert int(out['sizeof']) == ctypes.sizeof(_lib.PackJob)
    for f in fields:
        assert int(out[f]) == getattr(_lib.PackJob, f).offset, f
    assert _lib.PackJob.src_channels.size == ctypes.sizeof(ctypes.c_int) * int(out['DM_MAX_SOURCES'])


def test_the_abi_number_has_one_definition():
    from dynamask_amd import ops
    assert _lib.ABI_VERSION == 29
    assert len(re.findall(r'^#define DM_ABI_VERSION 29\b', open(HEADER).read(), flags=re.M)) == 1
    src = open(API_MISC).read()
    assert src.count('DM_ABI_VERSION') == 2 and '29' not in src       # dm_abi_version() and the dm_build_info() string
    assert not re.search(r'^ABI_VERSION\s*=', open(_lib.__file__).read(), flags=re.M)
    assert ops.AUG_VIEW_FLOATS == 8 and not re.search(r'^AUG_VIEW_FLOATS\s*=\s*\d', open(ops.__file__).read(), flags=re.M)
