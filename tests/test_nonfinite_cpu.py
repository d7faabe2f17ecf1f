"""Every entry of tests/nonfinite_cases.py::CASES can show a failure: the references alone, no GPU.  These are conditions on
the cases (planted positions, seeds, shapes), not measurements of anything: a case whose reference held no NaN, or whose
fp32 and float64 references disagreed on where the NaN is, would let tests/test_nonfinite_gpu.py pass on a wrong kernel
or fail on a right one."""
import pytest
import torch

import nonfinite_cases as nf


@pytest.mark.parametrize('case', nf.CASES, ids=[c.id for c in nf.CASES])
def test_the_reference_of_the_case_can_show_a_failure(case):
    ref32, ref64 = case.refs()
    assert ref32.dtype == torch.float32 and ref64.dtype == torch.float64 and ref32.shape == ref64.shape
    for name, a, b in zip(('NaN', '+Inf', '-Inf'), nf.classes(ref32), nf.classes(ref64)):
        assert torch.equal(a, b), f'{case.id}: the fp32 and the float64 reference differ in {int((a != b).sum())} {name} positions'
    nan, pinf, ninf = nf.classes(ref64)
    assert int(nan.sum()) >= 1, f'{case.id}: no NaN reaches the output'
    if case.can_inf:
        assert int(pinf.sum()) >= 1, f'{case.id}: no +Inf reaches the output'
    finite = torch.isfinite(ref64)
    assert int(finite.sum()) * 2 >= ref64.numel(), f'{case.id}: fewer than half of the outputs are finite'
    assert bool((ref64[finite] != 0).any()), f'{case.id}: the finite outputs are identically zero'


def test_plant_keeps_its_margin_and_writes_each_special_once():
    x = nf.plant(torch.zeros(4, 3, 7, 9), 'pixels', c=1)
    nan, pinf, ninf = nf.classes(x)
    assert (int(nan.sum()), int(pinf.sum()), int(ninf.sum())) == (1, 2, 2)
    bad = ~torch.isfinite(x)
    assert not bool(bad[:, :, :2].any() or bad[:, :, -2:].any() or bad[:, :, :, :2].any() or bad[:, :, :, -2:].any())
    assert [int(bad[i].sum()) for i in range(4)] == [1, 1, 1, 2] and bool(bad[:, 1].sum() == 5)
    y = nf.plant(torch.zeros(4, 3, 7, 9), 'channels')
    assert bool(torch.isinf(y[3, 0]).any() and torch.isinf(y[3, 1]).any()) and int((~torch.isfinite(y)).sum()) == 5


def test_assert_same_nonfinite_catches_an_erased_nan_and_a_moved_inf():
    ref = torch.tensor([1.0, nf.NAN, nf.INF, -nf.INF, 0.5], dtype=torch.float64)
    nf.assert_same_nonfinite(ref.float(), ref.float(), ref, 'same')
    for wrong in ([1.0, 0.0, nf.INF, -nf.INF, 0.5], [1.0, nf.NAN, nf.NAN, -nf.INF, 0.5], [1.0, nf.NAN, nf.INF, nf.INF, 0.5],
                  [nf.NAN, nf.NAN, nf.INF, -nf.INF, 0.5]):
        with pytest.raises(AssertionError, match='class differs'):
            nf.assert_same_nonfinite(torch.tensor(wrong), ref.float(), ref, 'wrong')
    with pytest.raises(AssertionError, match='allowed'):
        nf.assert_same_nonfinite(torch.tensor([1.0, nf.NAN, nf.INF, -nf.INF, 0.51]), ref.float(), ref, 'finite part')
