"""The typed call of hamgnn_amd/_lib.py on the device: a mistyped index tensor is refused before any launch, and strided() hands row-strided views on as they
are (pointer and row stride), bit-identical to contiguous copies."""
import pytest
import torch

from hamgnn_amd import _lib, nn as hnn, ops

pytestmark = pytest.mark.gpu


def test_segment_sum_refuses_an_int32_perm_before_any_launch(monkeypatch):
    msg = torch.randn(5, 8, device="cuda")
    rowptr = torch.tensor([0, 2, 2, 5], device="cuda")
    perm = torch.tensor([4, 0, 3, 1, 2], device="cuda")
    want = torch.stack([msg[[4, 0]].sum(0), torch.zeros(8, device="cuda"), msg[[3, 1, 2]].sum(0)])
    assert torch.allclose(ops.segment_sum(msg, rowptr, perm, 3), want, atol=1e-6)
    launches = []
    fn, convs, has_stream = _lib._bound["hg_segment_sum"]
    monkeypatch.setitem(_lib._bound, "hg_segment_sum", (lambda *a: launches.append(a) or 0, convs, has_stream))
    with pytest.raises(ValueError, match="hg_segment_sum: perm"):
        ops.segment_sum(msg, rowptr, perm.int(), 3)
    assert not launches
    ops.segment_sum(msg, rowptr, perm, 3)
    assert len(launches) == 1                                  # (the spy sees the launches that do happen)


def test_add_rows_takes_column_windows_as_they_are():
    torch.manual_seed(0)
    bufs = [torch.randn(33, 40, device="cuda") for _ in range(3)]
    a, b, c = (t[:, 8:32] for t in bufs)                       # [33, 24] windows of [33, 40] rows: one full and one ragged row group
    assert not a.is_contiguous()
    before = [t.clone() for t in bufs]
    for views in ((a, b), (a, b, c)):
        got = ops.add_rows(*views)
        want = ops.add_rows(*(v.contiguous() for v in views))
        assert got.is_contiguous() and torch.equal(got, want) and torch.equal(got, sum(views[1:], views[0]))      # (the kernel adds in this order: exact)
    assert all(torch.equal(t, t0) for t, t0 in zip(bufs, before))


def test_linear_planar_takes_row_strided_residuals_without_a_copy(monkeypatch):
    torch.manual_seed(1)
    lin = hnn.E3Linear("5x0e+7x0e+3x1o", "9x0e+2x1o+4x1o").compile("cuda")      # the smallest o3.Linear of the suite (tests/test_plan_emu.py)
    dl = lin._dp
    assert isinstance(dl, ops.DeviceLinear)
    rows = 37                                                  # a block of 32 rows and a ragged one
    x = torch.randn(rows, dl.in_dim, device="cuda")
    wide = [torch.randn(rows, dl.out_dim + 8, device="cuda") for _ in range(2)]
    views = [w[:, 4:4 + dl.out_dim] for w in wide]
    assert not any(v.is_contiguous() for v in views)
    seen = []
    real = ops.call
    monkeypatch.setattr(ops, "call", lambda name, *a, **kw: seen.append(a) or real(name, *a, **kw))
    got = ops.linear_planar(dl, x, res=views)
    want = ops.linear_planar(dl, x, res=[v.contiguous() for v in views])
    assert torch.equal(got, want)
    assert torch.allclose(got, ops.linear_planar(dl, x) + views[0] + views[1], atol=1e-5)      # (values of a few units: some fp32 ulps for the order of the adds)
    res_args = seen[0][7:11]                                   # (res0, res0_stride, res1, res1_stride) of the first launch
    for v, s, stride in zip(views, res_args[0::2], res_args[1::2]):
        assert type(s) is _lib.strided and s.t.data_ptr() == v.data_ptr() and stride == v.stride(0) == dl.out_dim + 8
