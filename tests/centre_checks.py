"""Checks of the centre-only edge sources of the first layer (hamgnn_conv._centre_edge_set, plan.build_message_pack_program(centre_edge=...)): shared by the CPU
tests (planner emulator, host code on the stand-ins) and the `-m gpu` tests."""
import os

import numpy as np
import torch

from hamgnn_amd import plan as P
from hamgnn_amd import so3
from tests import gpu_checks as G


def first_layer_sets(irr, sh):
    """(zero_node, zero_edge, centre_edge) of a backbone's first layer for node / edge irreps `irr` and spherical harmonics `sh`, worked out here from the
    irreps alone (not through the model): 0e node rows; edge rows hold the irreps of the Y^l, those with l > 0 in their m = 0 component only"""
    I = so3.Irreps(irr)
    shs = {(l, p) for _, l, p in so3.Irreps(sh)}
    return (tuple(i for i, (_, l, p) in enumerate(I) if (l, p) != (0, 1)), tuple(i for i, (_, l, p) in enumerate(I) if (l, p) not in shs),
            tuple(i for i, (_, l, p) in enumerate(I) if (l, p) in shs and l > 0))


def first_layer_rows(irr, sh, E, seed, node_full):
    """planar (sender rows, receiver rows, edge rows) as a first layer sees them: edge rows zero outside the irreps of the Y^l and, for l > 0, outside the
    centre component; node rows 0e only unless node_full (a PairInteractionBlock reads the updated node rows)"""
    lay = P.PlanarLayout(irr)
    zn, ze, ce = first_layer_sets(irr, sh)
    rng = np.random.default_rng(seed)
    xs, xd, fe = (np.zeros((E, lay.dim)) for _ in range(3))
    for i, (mul, l, p) in enumerate(lay.irreps):
        o, mp = lay.off[i], lay.mulp[i]
        for a in range(2 * l + 1):
            if node_full or i not in zn:
                xs[:, o + a * mp:o + a * mp + mul] = rng.normal(size=(E, mul))
                xd[:, o + a * mp:o + a * mp + mul] = rng.normal(size=(E, mul))
            if i not in ze and (i not in ce or a == l):
                fe[:, o + a * mp:o + a * mp + mul] = rng.normal(size=(E, mul))
    return xs, xd, fe


def check_centre_zeros(device="cuda", legacy=False, charge=False, irr=None, sh=None, radial=(16, 16), num_radial=8, graph=None, n_atoms=9, seed=11, num_layers=2):
    """the backbone with the centre-only programs of its first layer against the SAME model compiled with HG_CENTRE_ZEROS=0 (the irrep-level shortcut alone)
    and with HG_STRUCT_ZEROS=0 (every path of the reference issued), HG_CHECK_STRUCT_ZEROS=1 throughout (the marked entries of the embeddings' rows ARE zero).
    Returns the node / edge row differences, what the launches of the reduced forward were (kernel, parts, fused scatter), the tile statistics of the graph
    and the issued-MFMA ratios of the first ConvBlock / first PairInteractionBlock programs."""
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.models.hamgnn_conv import HamGNNConvE3
    cfg = dict(num_types=96, irreps_edge_sh=sh or G.SH, edge_sh_normalization="component", edge_sh_normalize=True, build_internal_graph=False,
               cutoff=26.0, rbf_func="bessel", num_radial=num_radial, num_layers=num_layers, irreps_node_features=irr or G.MINI, use_kan=False,
               radial_MLP=list(radial), correlation=2, num_hidden_features=4, use_corr_prod=False, legacy_edge_update=legacy)
    if charge:
        cfg.update(apply_charge_doping=True, num_charge_attr_feas=8)
    torch.manual_seed(seed)
    m = HamGNNConvE3(cfg)
    g = graph if graph is not None else S.random_cell(n_atoms, [14, 8, 6, 1], seed=seed, density=0.004)
    if charge:
        g["doping_charge"] = torch.tensor(0.7)
    g = g.to(device)
    E = int(g.num_edges)
    out = dict(G.tile_statistics(g.edge_index[1], int(g.num_nodes)))
    reps, mfma, centre = {}, {}, {}
    os.environ["HG_CHECK_STRUCT_ZEROS"] = "1"
    try:
        for tag, env in (("centre", {}), ("irrep", {"HG_CENTRE_ZEROS": "0"}), ("complete", {"HG_STRUCT_ZEROS": "0"})):
            os.environ.update(env)
            try:
                if tag != "centre":
                    m.compile(torch.device(device))
                with G.spy_tp_fused() as launches, torch.no_grad():
                    reps[tag] = m(g)
                if tag == "centre":
                    out["launches"] = [(l["kernel"], str(l["parts"]), bool(l["reduce"])) for l in launches if l.get("tag", "message_pack") == "message_pack"]
                blocks = (m.convolutions[0].conv_tp, m.pair_interactions[0].conv_tp, m.pair_interactions[-1].conv_tp)
                mfma[tag] = [int(b._dp_for(E, True).prog.mfma_per_wave) for b in blocks]
                centre[tag] = [tuple(b.conv_tp._zkw_compiled.get("centre_edge", ())) for b in (*m.convolutions, *m.pair_interactions)]
            finally:
                for k in env:
                    os.environ.pop(k, None)
    finally:
        os.environ.pop("HG_CHECK_STRUCT_ZEROS", None)
    if device != "cpu":
        torch.cuda.synchronize()
    for tag in ("irrep", "complete"):
        out[f"node_rel_err_vs_{tag}"] = G.rel(reps["centre"]["node_attr"], reps[tag]["node_attr"])
        out[f"edge_rel_err_vs_{tag}"] = G.rel(reps["centre"]["edge_attr"], reps[tag]["edge_attr"])
    out["first_conv_mfma_ratio"] = mfma["centre"][0] / mfma["irrep"][0]
    out["first_pair_mfma_ratio"] = mfma["centre"][1] / mfma["irrep"][1]
    out["last_pair_mfma_ratio"] = mfma["centre"][2] / mfma["irrep"][2]
    out["centre_sets"], out["centre_sets_switched_off"] = centre["centre"], centre["irrep"]
    return out
