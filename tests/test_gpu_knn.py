"""exact k nearest rows (fp_knn_l2) against a float64 brute force."""
import numpy as np
import pytest
import torch

from tests import _clip_ref as cr

pytestmark = pytest.mark.gpu


def _case(N, E, Q, k, dup):
    """queries = unit vectors; table rows sit around the queries at well separated squared distances.  Drawn (first seed that
    qualifies) so that, per query, the float64 gap between consecutive sorted distances among the k + 1 nearest exceeds the fp32
    bound 2 E 2^-24 (|a|^2 + |b|^2) — except between the planted exact duplicates, which must come out in index order."""
    for seed in range(40):
        rng = np.random.Generator(np.random.PCG64(1000 * N + E + 7 * Q + k + 100000 * seed))
        q = rng.standard_normal((Q, E))
        q /= np.linalg.norm(q, axis=1, keepdims=True)
        u = rng.standard_normal((N, E))
        u /= np.linalg.norm(u, axis=1, keepdims=True)
        a2 = 0.05 * (1 + np.arange(N) // Q) * (1 + 0.2 * rng.random(N))
        t = q[np.arange(N) % Q] + np.sqrt(a2)[:, None] * u
        t, q = t.astype(np.float32), q.astype(np.float32)
        pairs = []
        if dup:                                  # rows 0 and Q are the two nearest rows of query 0: copy them to later rows
            for src, dst in ((0, N - 1), (Q if N > Q else 0, N - 2)):
                t[dst] = t[src]
                pairs.append((src, dst))
        idx, d2 = cr.knn_f64(t, q, min(k + 1, N))
        ok = True
        for j in range(Q):
            d = d2[j, idx[j]]
            for m in range(len(d) - 1):
                a, b = idx[j, m], idx[j, m + 1]
                if np.array_equal(t[a], t[b]):
                    continue
                bound = 2 * E * 2.0 ** -24 * ((t[a].astype(np.float64) ** 2).sum() + (t[b].astype(np.float64) ** 2).sum() + 2 * (q[j].astype(np.float64) ** 2).sum())
                ok &= (d[m + 1] - d[m]) > bound
        if ok:
            return t, q, idx[:, :k], d2, pairs
    raise AssertionError("no seed gives separated distances")


def test_entry_point_is_exported():
    from freepose_amd import _lib
    assert hasattr(_lib.load(), "fp_knn_l2") and hasattr(_lib.load(), "fp_op_attention_hd")


@pytest.mark.parametrize("dup", [False, True], ids=["plain", "duplicates"])
@pytest.mark.parametrize("k", [1, 11])
@pytest.mark.parametrize("Q", [1, 5])
@pytest.mark.parametrize("E", [64, 1280])
@pytest.mark.parametrize("N", [11, 12, 1000])
def test_knn_l2(N, E, Q, k, dup):
    from freepose_amd import ops
    t, q, ref_idx, d2, pairs = _case(N, E, Q, k, dup)
    idx, dist = ops.knn_l2(torch.from_numpy(t), torch.from_numpy(q), k)
    idx, dist = idx.cpu().numpy(), dist.cpu().numpy()
    assert np.array_equal(idx, ref_idx)
    ref_d = np.take_along_axis(d2, ref_idx, axis=1)
    assert np.allclose(dist, ref_d, rtol=1e-4, atol=1e-6)
    if dup and k > 1:
        row = idx[0].tolist()
        for src, dst in pairs:
            if src in row and dst in row:
                assert row.index(dst) == row.index(src) + 1, "exact duplicates come out in index order, side by side"
        assert any(src in row and dst in row for src, dst in pairs)
    idx2, dist2 = ops.knn_l2(torch.from_numpy(t), torch.from_numpy(q), k)
    assert torch.equal(idx2.cpu(), torch.from_numpy(idx)) and torch.equal(dist2.cpu(), torch.from_numpy(dist))


def test_knn_l2_refusals():
    from freepose_amd import ops
    t, q = torch.zeros((10, 8)), torch.zeros((2, 8))
    for k in (0, 11, 65):
        with pytest.raises(RuntimeError, match="knn_l2"):
            ops.knn_l2(t, q, k)
    with pytest.raises(ValueError):
        ops.knn_l2(t, torch.zeros((2, 9)), 1)
