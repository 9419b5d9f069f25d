"""The hand-made two-crystal batch on which kspace.CrystalTables is pinned (tests/test_kspace_tables_cpu.py, tests/test_kspace_tables_gpu.py): every case of the
index plumbing in the fewest atoms, nao 13 (openmx), 3 k-points per crystal.
  crystal A: C, H (H lacks 8 of the 13 orbitals: orank has -1 entries), one bond in both directions and a self image of the C atom
  crystal B: C, O, H with two edges C -> O that differ only in the shift, a self-image edge (H, H, shift != 0), no edge between C and H in either direction,
             and an edge list that is NOT sorted by atom pair (the stable sort of the pair tables has work to do)
Hermitian-consistent random rows through inv_edge_idx, S(k) positive definite (unit on-site blocks + 0.004 noise, as sharded_losses_checks.band_graph)."""
import numpy as np
import torch

NAO, NK = 13, 3
A = ([6, 1], [(0, 1, (0, 0, 0)), (0, 0, (1, 0, 0)), (1, 0, (0, 0, 0)), (0, 0, (-1, 0, 0))])
B = ([6, 8, 1], [(0, 1, (1, 0, 0)), (2, 2, (0, 1, 0)), (1, 0, (0, 0, 0)), (0, 1, (0, 0, 0)), (1, 2, (0, 0, 0)), (2, 1, (0, 0, 0)), (1, 0, (-1, 0, 0)),
                 (2, 2, (0, -1, 0))])


def crystal(spec, seed, soc=False):
    """one crystal of the batch as a Graph with random targets, overlaps and overlap gradients"""
    from hamgnn_amd.data import synthetic as S
    from hamgnn_amd.data.graph import Graph
    z, edges = spec
    n, e = len(z), len(edges)
    cell = 9.0 * np.eye(3) + 0.3 * np.arange(9).reshape(3, 3) / 8.0
    sh = np.array([s for _, _, s in edges], dtype=np.int64)
    inv = np.array([edges.index((j, i, tuple(-v for v in s))) for i, j, s in edges], dtype=np.int64)
    g = Graph(z=torch.tensor(z), pos=torch.zeros(n, 3), cell=torch.from_numpy(cell.astype(np.float32))[None],
              edge_index=torch.tensor([[i for i, _, _ in edges], [j for _, j, _ in edges]]), cell_shift=torch.from_numpy(sh),
              nbr_shift=torch.from_numpy((sh @ cell).astype(np.float32)), inv_edge_idx=torch.from_numpy(inv), batch=torch.zeros(n, dtype=torch.long),
              node_counts=torch.tensor([n]))
    S.add_random_targets(g, NAO, seed=seed, soc=soc)
    gen = torch.Generator().manual_seed(seed + 71)
    so = 0.004 * torch.randn(e, NAO, NAO, generator=gen)
    g["Soff"] = (0.5 * (so + so[g.inv_edge_idx].transpose(1, 2))).reshape(e, -1)
    sn = 0.004 * torch.randn(n, NAO, NAO, generator=gen)
    g["Son"] = (torch.eye(NAO) + 0.5 * (sn + sn.transpose(1, 2))).reshape(n, -1)
    g["dSon"], g["dSoff"] = 0.1 * torch.randn(n, NAO * NAO, 3, generator=gen), 0.1 * torch.randn(e, NAO * NAO, 3, generator=gen)
    g["k_vecs"] = 0.05 * torch.randn(1, NK, 3, generator=gen)
    return g


def batch(soc=False):
    """crystals A and B collated, k_vecs [2, NK, 3]"""
    from hamgnn_amd.data import collate
    parts = [crystal(A, 11, soc), crystal(B, 12, soc)]
    g = collate(parts)
    for k in ("dSon", "dSoff", "k_vecs"):
        g[k] = torch.cat([p[k] for p in parts], 0)
    return g


def head(device):
    """the smallest head of the fixtures (scalar features, nao 13), compiled: the k-space step reads its basis tables only"""
    from hamgnn_amd.models.hamgnn_output import HamGNNPlusPlusOut
    return HamGNNPlusPlusOut("4x0e", "4x0e", nao_max=NAO, ham_type="openmx", ham_only=True, symmetrize=True, add_H0=False, soc_switch=False,
                             calculate_band_energy=True, num_k=NK, k_path=None, calculate_sparsity=False).compile(device)


def check_built_once(device, monkeypatch):
    """band_energies_soc and band_energy_backward_soc on the batch: constructions of CrystalTables, sorts of its pair tables and assembly launches, counted"""
    from hamgnn_amd import kspace
    g = batch(soc=True).to(device)
    hd = head(device)
    built, sorted_, launches = [], [], []
    from_graph, sort, real = kspace.CrystalTables.from_graph.__func__, torch.sort, kspace.ops.hk_assemble
    monkeypatch.setattr(kspace.CrystalTables, "from_graph", classmethod(lambda cls, *a: built.append(1) or from_graph(cls, *a)))
    monkeypatch.setattr(torch, "sort", lambda *a, **kw: sorted_.append(1) or sort(*a, **kw))      # (the pair tables' stable sort is the step's only one)
    monkeypatch.setattr(kspace.ops, "hk_assemble", lambda *a: launches.append(1) or real(*a))
    rows = [g[k] for k in ("Hon", "iHon", "Hoff", "iHoff")]
    be, wf = kspace.band_energies_soc(hd, *rows, g)
    assert (len(built), len(sorted_), len(launches)) == (2, 2, 18)
    assert tuple(be.shape) == (2 * (18 + 31), NK) and bool(torch.isfinite(be).all())
    grads = kspace.band_energy_backward_soc(hd, *rows, g, torch.ones_like(be))
    assert (len(built), len(sorted_), len(launches)) == (4, 4, 36)
    assert all(tuple(a.shape) == tuple(r.shape) and bool(torch.isfinite(a).all()) for a, r in zip(grads, rows)) and float(grads[2].abs().max()) > 0
