"""-m gpu: the epilogue of the edge kernel (csrc/tp_stage.h:epilogue_is, lane map csrc/tp_epilogue_map.h) on the narrow and ragged segments where its lane groups
take different output components in one wave step.  One MessagePackBlock whose output irreps hold 2, 4, 9, 12, 18 and 25 channels at l = 1 .. 3 (the largest l of the
mini harmonics) plus l = 0, on 24 edges -- one full 16-edge tile and a last tile of 8 -- in the three forms the epilogue has:
  reduce: un-rotated output, fused receiver scatter, receivers 5 + 14 + 5 edges: the middle run crosses the tile boundary;
  edge  : edge-frame output (the plain copy a PairInteractionBlock's launch takes);
  split : eight workgroups per tile (`tp_is_kernel<true, false>`).
Each against the fp64 oracle under G.TOL (1e-5 relative to the largest element, the bound of the parity tests of these launches), and launched twice: bit-identical.
The set-A block on the 172 edges of the primitive Si cell passes the same way."""
import os

import numpy as np
import pytest
import torch

from tests import gpu_checks as G

pytestmark = pytest.mark.gpu

IRR = "25x0e+9x0o+2x1o+18x1e+4x2e+25x2o+9x3o+12x3e"
SH = "0e+1o+2e+3o"


@pytest.fixture(scope="module", autouse=True)
def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")


def graph24():
    """24 edges on 3 receivers, receiver-sorted runs of 5, 14 and 5 edges (slots 0-4, 5-18, 19-23), the edges themselves in a shuffled order"""
    rng = np.random.default_rng(7)
    dst = rng.permutation(np.repeat(np.arange(1, 4), [5, 14, 5]).astype(np.int64))
    return 5, rng.integers(0, 5, size=24), dst


def graph_si2():
    from hamgnn_amd.data import synthetic as S
    g = S.si_diamond(primitive=True)
    ei = g["edge_index"].numpy()
    return int(g["z"].shape[0]), ei[0].copy(), ei[1].copy()


def run_block(form, irr, sh, graph, radial=(16, 16), seed=3, device="cuda"):
    """the launch of `form` twice, and the fp64 oracle's rows: (y1, y2, want, launch record)"""
    from oracle import hamgnn_ref as R, e3
    from hamgnn_amd import nn as hnn, ops, plan as P
    from hamgnn_amd.topo import Topology
    N, src_np, dst_np = graph
    E = int(dst_np.size)
    s_, r_ = torch.from_numpy(src_np), torch.from_numpy(dst_np)
    lmax, lsh = P.Irreps(irr).lmax, P.Irreps(sh).lmax
    torch.manual_seed(seed)
    prev = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        ref = R.MessagePackBlock(irr, irr, sh, irr, "8x0e", radial_MLP=list(radial))
        g = torch.Generator().manual_seed(seed)
        D = ref.irreps_node_feats.dim
        xs, xd, ef = torch.randn(N, D, generator=g), torch.randn(N, D, generator=g), torch.randn(E, D, generator=g)
        n = torch.nn.functional.normalize(torch.randn(E, 3, generator=g), dim=-1)
        shv = e3.spherical_harmonics(list(range(lsh + 1)), n, True, "component")
        rbf = torch.randn(E, 8, generator=g)
        with torch.no_grad():
            want = ref(xs[s_], xd[r_], ef, shv, rbf)
            if form == "reduce":
                want = torch.zeros(N, D).index_add_(0, r_, want)
    finally:
        torch.set_default_dtype(prev)
    m = G.load_weights(hnn.MessagePackBlock(irr, irr, sh, irr, 8, list(radial)), {k: v.detach().numpy() for k, v in ref.state_dict().items()})
    lay = P.PlanarLayout(irr)
    lm = max(lmax, lsh)
    v = torch.stack([n[:, 2], n[:, 0], n[:, 1]], 1) * 2.0          # e3nn axis order (y, z, x) -> physical (x, y, z)
    jtab = torch.from_numpy(P.wigner_jtab(lm)).to(device)
    ei = torch.stack([s_, r_]).to(device)
    imap = torch.from_numpy(lay.index_map().astype(np.int32)).to(device)
    rot = torch.from_numpy(P.rotate_table(lay)).to(device)
    pl = lambda t: ops.to_planar(t.float().to(device), imap, lay.dim)
    os.environ["HG_IS_PARTS"] = "8" if form == "split" else "1"
    try:
        m.compile(device, unrotate=form != "edge")
        geo = ops.Geometry(torch.zeros(N, 3, device=device), ei, v.float().to(device), 8.0, 8, lm, jtab)
        geo.rbf = rbf.float().to(device).contiguous()
        f_rot = ops.rotate_gather(pl(ef), None, geo, rot)
        nodes_s, nodes_d = pl(xs), pl(xd)
        topo = Topology({"edge_index": ei, "z": torch.zeros(N, dtype=torch.long, device=device)})
        assert m._dp_for(E).fixed_parts is None, "the block's tiles do not fit one workgroup: not the launch this test is about"

        def launch():
            if form == "reduce":
                eperm, run_id, R_, prow, ident = topo.receiver_major()
                return ops.segment_sum(m.run_nodes(nodes_s, nodes_d, f_rot, geo, rot, reduce=(eperm, run_id, R_)), prow, ident, N)
            y = m.run_nodes(nodes_s, nodes_d, f_rot, geo, rot)
            return ops.rotate_gather(y, None, geo, rot, transpose=True) if form == "edge" else y

        with G.spy_tp_fused() as launches:
            y1 = ops.from_planar(launch(), imap).clone()
            y2 = ops.from_planar(launch(), imap).clone()
    finally:
        os.environ.pop("HG_IS_PARTS", None)
    torch.cuda.synchronize()
    assert len(launches) == 2, launches
    return y1, y2, want, launches[0]


def _check(form, y1, y2, want, l):
    err = G.rel(y1, want)
    print({"form": form, "launch": l, "rel_err": err, "out_max_abs": want.abs().max().item(), "elements_changed_on_repeat": int((y1 != y2).sum())})
    assert l["kernel"] == "is" and l["reduce"] == (form == "reduce"), l
    assert (l["parts"] == 1) == (form != "split"), l
    assert torch.equal(y1, y2)
    assert bool(torch.isfinite(y1).all()) and err < G.TOL, err


@pytest.mark.parametrize("form", ["reduce", "edge", "split"])
def test_epilogue_narrow_and_ragged_segments_24_edges(form):
    _check(form, *run_block(form, IRR, SH, graph24()))


@pytest.mark.parametrize("form", ["reduce", "edge", "split"])
def test_epilogue_set_a_block_si2(form):
    import bench
    _check(form, *run_block(form, bench.IRREPS["A"], bench.SH, graph_si2(), radial=(64, 64)))
