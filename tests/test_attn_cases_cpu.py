"""The claims of tests/_attn_cases.py, proven without a GPU: the shape lists reach every dispatch branch of the three attention kernels,
the select preconditions hold at every listed shape, every input is bf16-exact, the float64 references agree with exact rational
arithmetic, and the bf16-neighbour rule is right at ties, powers of two and zero."""
from fractions import Fraction

import numpy as np
import pytest

from tests import _attn_cases as ac


# ---- coverage ---------------------------------------------------------------------------------------------------------------------------


def test_dino_shape_list_reaches_every_branch():
    assert {n for _, _, n in ac.DINO_SHAPES} == set(ac.DINO_NTOK)
    assert {(B, H) for B, H, _ in ac.DINO_SHAPES} == set(ac.DINO_BH)
    assert all(B * H <= 7 and n <= 321 for B, H, n in ac.DINO_SHAPES)
    d = {s: ac.dino_dispatch(*s) for s in ac.DINO_SHAPES}
    table = {
        "short_tail": [s for s, x in d.items() if x.short_tail],
        "full_tail": [s for s, x in d.items() if not x.short_tail],
        "clamped_last_tile": [s for s, x in d.items() if x.clamped_last],
        "unclamped_last_tile": [s for s, x in d.items() if not x.clamped_last],
        "partial_tile_without_pad_rows": [s for s, x in d.items() if x.partial_full_pad],
        "odd_tile_count": [s for s, x in d.items() if x.ntile_odd],
        "even_tile_count": [s for s, x in d.items() if not x.ntile_odd],
        "odd_tile_count_short": [s for s, x in d.items() if x.ntile_odd and x.short_tail],
        "even_tile_count_short": [s for s, x in d.items() if not x.ntile_odd and x.short_tail],
        "idle_wave": [s for s, x in d.items() if x.idle_waves],
        "half_stored_wave": [s for s, x in d.items() if x.half_waves],
        "several_query_blocks": [s for s, x in d.items() if x.npad > ac.DINO_QB],
        **{f"nwg_mod8_{r}": [s for s, x in d.items() if x.nwg_mod8 == r and 1 <= x.nwg <= 21] for r in range(8)},
    }
    empty = [name for name, shapes in table.items() if not shapes]
    assert not empty, f"no shape reaches: {empty}"
    # every listed shape runs both the plain and the pre-scaled kernel, so pre-scaled x short_tail is complete when both tails exist
    names = [n for n, _ in ac.dino_cases()]
    for B, H, n in ac.DINO_SHAPES:
        for fam in ("select-plain", "select-pre", "uniform-plain", "uniform-pre", "pow2-pre", "nat8-plain"):
            assert f"{fam}-B{B}H{H}n{n}" in names
    assert {n for _, _, n in table["partial_tile_without_pad_rows"]} >= {16, 32, 96, 160}
    assert all(1 <= x.nwg <= 21 for x in d.values())
    assert set(ac.DINO_PAD_NTOK) <= set(ac.DINO_NTOK) and all(ac.pad16(n) > n for n in ac.DINO_PAD_NTOK)


def test_dino_dispatch_mirror_by_hand():
    x = ac.dino_dispatch(1, 6, 905)       # ViT-L @ 420: 14 full tiles + 9 keys
    assert (x.npad, x.ntile, x.short_tail, x.clamped_last, x.idle_waves, x.half_waves, x.nwg) == (912, 15, True, True, 3, 1, 48)
    assert x.tile_order[:3] == (14, 0, 1)
    x = ac.dino_dispatch(2, 2, 64)
    assert (x.npad, x.ntile, x.short_tail, x.clamped_last, x.partial_full_pad, x.idle_waves, x.half_waves) == (64, 1, False, False, False, 2, 0)
    x = ac.dino_dispatch(1, 1, 96)        # tail of exactly 32 keys is still short; npad == n_tok with a partial tile
    assert x.short_tail and x.partial_full_pad and x.clamped_last and x.tile_order == (1, 0)
    assert not ac.dino_dispatch(1, 1, 97).short_tail and not ac.dino_dispatch(1, 1, 32).short_tail
    assert ac.dino_dispatch(1, 1, 1).half_waves == 1 and ac.dino_dispatch(1, 1, 1).idle_waves == 3


@pytest.mark.parametrize("nwg", range(1, 22))
def test_xcd_remap_is_a_bijection(nwg):
    assert sorted(ac.xcd_remap(nwg)) == list(range(nwg))


def test_dispatch_mirror_against_the_kernel_header(tmp_path):
    """tools/attn_host_check.cpp — csrc/attn_core.h, the functions attention.hip and its launcher call — built with
    -fsanitize=address,undefined as a stand-alone program: its own checks pass (block remap, tile order, LDS maps replayed on a labelled
    host image, clamped staging, mask, wait ladder), and the dispatch records it prints are what dino_dispatch / xcd_remap say"""
    import shutil
    import subprocess
    from pathlib import Path
    root = Path(__file__).resolve().parent.parent
    gxx = shutil.which("g++")
    assert gxx, "g++ not found"
    exe = tmp_path / "attn_host_check"
    r = subprocess.run([gxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-I", str(root / "freepose_amd" / "csrc"),
                        str(root / "tools" / "attn_host_check.cpp"), "-o", str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-3000:]
    shapes = list(ac.DINO_SHAPES) + [(B, H, n) for B, H in ((1, 1), (2, 3)) for n in range(1, 2049)]
    args = [f"{B},{H},{n}" for B, H, n in ac.DINO_SHAPES] + ["1,1,1-2048", "2,3,1-2048"]
    r = subprocess.run([str(exe), *args], capture_output=True, text=True)
    assert r.returncode == 0 and "attn_host_check: ok" in r.stdout, (r.returncode, r.stdout[-2000:], r.stderr[-3000:])
    lines = [ln for ln in r.stdout.splitlines() if ln.startswith("dispatch ")]
    assert len(lines) == len(shapes)
    for (B, H, n), ln in zip(shapes, lines):
        head, order, remap = (part.split() for part in ln.split("|"))
        d = ac.dino_dispatch(B, H, n)
        assert [int(x) for x in head[1:]] == [B, H, n, d.npad, d.ntile, d.short_tail, d.clamped_last, d.idle_waves, d.half_waves, d.nwg], ln[:120]
        assert tuple(int(x) for x in order) == d.tile_order, (B, H, n)
        assert [int(x) for x in remap] == ac.xcd_remap(d.nwg), (B, H, n)
    # the kernel and its launcher take these from the header, not from expressions of their own
    src = (root / "freepose_amd" / "csrc" / "attention.hip").read_text()
    for fn in ("fp_attn_product_flavour", "fp_attn_grid", "fp_attn_block_remap", "fp_attn_block_of", "fp_attn_wave_q0", "fp_attn_wave_idle", "fp_attn_num_tiles",
               "fp_attn_tile_of", "fp_attn_in_flight", "fp_attn_stage_clamped", "fp_attn_clamp_key", "fp_attn_clamp_group", "fp_attn_dma_row", "fp_attn_dma_base",
               "fp_attn_dma_kchunk", "fp_attn_dma_vchunk", "fp_attn_frag_chunk", "fp_attn_kfrag_step", "fp_attn_vfrag_step", "fp_attn_acc_key"):
        assert fn + "(" in src, fn


def test_hd_and_causal_shape_lists_reach_every_branch():
    hd = {(d, n): ac.hd_dispatch(d, n) for d in ac.HD_DIMS for n in ac.HD_NTOK}
    assert {x.nkk for x in hd.values()} == {1, 2, 3, 4}
    assert any(x.hd_padded for x in hd.values()) and any(not x.hd_padded for x in hd.values())
    assert any(x.idle_waves for x in hd.values()) and any(x.idle_waves == 0 for x in hd.values())
    assert any(x.partial_tile for x in hd.values()) and any(not x.partial_tile for x in hd.values())
    assert {x.ntile for x in hd.values()} >= {1, 2, 3, 5} and {x.nqb for x in hd.values()} >= {1, 2, 3, 5}
    ca = {(d, n): ac.hd_dispatch(d, n) for d in ac.CAUSAL_DIMS for n in ac.CAUSAL_NTOK}
    assert {x.nkk for x in ca.values()} == {1, 2, 4}      # 8, 64, 104 -> 1, 2, 4 k steps
    assert any(x.causal_skipped for x in ca.values()) and any(x.causal_skipped == 0 for x in ca.values())
    assert ca[(64, 77)].causal_tiles == (1, 2) and ca[(64, 77)].causal_skipped == 1
    assert ca[(8, 130)].causal_tiles == (1, 2, 3) and ca[(8, 130)].causal_skipped == 3
    assert ca[(8, 64)].causal_tiles == (1,) and ca[(8, 65)].causal_tiles == (1, 2)
    sel = [n for n, _ in ac.hd_cases() if n.startswith("select")]
    assert all("hd8n" not in n for n in sel) and len(sel) == 4 * len(ac.HD_NTOK)
    assert len(ac.hd_cases()) == 2 * 5 * len(ac.HD_NTOK) + len(sel)
    assert len(ac.causal_cases()) == 2 * 3 * len(ac.CAUSAL_NTOK) + 2 * len(ac.CAUSAL_NTOK)


def test_one_hot_layout_has_quiet_and_mixed_ballots():
    """the lazy test of attention.hip is a ballot over one 16-query half: both a half that never asks for a rescale after the first tile
    and a half that mixes such queries with rescaling ones must occur, on the short-tail and the full-tail order, in pow2 and nat8"""
    for build in (lambda B, H, n: ac.pow2_case("dino", B, H, 64, n), ac.nat8_case):
        for want_short in (False, True):
            quiet = mixed = 0
            for B, H, n in ac.DINO_SHAPES:
                if ac.dino_dispatch(B, H, n).short_tail == want_short and n > 64:
                    a, b = ac.half_census(build(B, H, n))
                    quiet, mixed = quiet + a, mixed + b
            assert quiet > 0 and mixed > 0


def test_profiles_sit_on_both_sides_of_the_threshold():
    rng = np.random.default_rng(0)
    for under, over, thr in ((7, 8, ac.THR2), (5, 6, ac.THR_NAT)):
        assert under <= thr < over and 2 * under > thr
        L = ac.profile_table(321, 336, under, over, rng)
        order = tuple(range(6))
        assert ac.lazy_rescales(L[:321, 2], 321, thr, order) == 2     # steps of `under`: tiles 2 and 4 move the reference
        assert ac.lazy_rescales(L[:321, 3], 321, thr, order) == 5     # steps of `over`: every tile
        assert ac.lazy_rescales(L[:321, 4], 321, thr, order) == 0 and ac.lazy_rescales(L[:321, 5], 321, thr, order) == 0
        assert ac.lazy_rescales(L[:321, 6], 321, thr, order) == 1     # the `under` key passes, the `over` key does not
        assert ac.lazy_rescales(L[:321, 7], 321, thr, order) == 1 and ac.lazy_rescales(L[:321, 8], 321, thr, order) == 0
        short = (5, 0, 1, 2, 3, 4)                                    # tail tile first: a rising profile starts from its top
        assert ac.lazy_rescales(L[:321, 3], 321, thr, short) == 0 and ac.lazy_rescales(L[:321, 4], 321, thr, short) == 1
        assert np.abs(L).max() <= 200


# ---- inputs -----------------------------------------------------------------------------------------------------------------------------

ALL_CASES = [("dino-" + n, f) for n, f in ac.dino_cases()] + [("hd-" + n, f) for n, f in ac.hd_cases()] + \
            [("causal-" + n, f) for n, f in ac.causal_cases()]


def test_every_case_builds_and_is_bf16_exact():
    """builds every case (the select builder asserts its preconditions: minimum Hamming distance >= 8, float64 softmax within 2^-20 of
    V[pi(t)]); every finite q, k, v value survives bf16; pads are what the families promise"""
    worst_dev, least_ham = 0.0, 1 << 30
    for name, build in ALL_CASES:
        c = build()
        for a in (c.q, c.k, c.v):
            assert a.shape == (c.B, c.H, c.npad, c.hd) and ac.bf16_exact(a), name
        assert np.isfinite(c.q[:, :, :c.n_tok]).all() and np.isfinite(c.k[:, :, :c.n_tok]).all() and np.isfinite(c.v).all(), name
        assert c.expected.shape == (c.B, c.H, c.n_tok, c.hd) and np.isfinite(c.expected).all(), name
        if c.kernel == "dino":
            assert np.isfinite(c.q).all(), name            # attention.hip reads its pad query rows
            qk, vt = ac.pack_qk_vt(c)
            assert qk.shape == (c.B * c.npad, 2 * c.H * 64) and vt.shape == (c.B, c.H, 64, c.npad)
        else:
            assert ac.pack_qkv(c).shape == (c.B, c.npad, 3 * c.H * c.hd)
        if c.family == "select":
            worst_dev, least_ham = max(worst_dev, c.info["ref_dev"]), min(least_ham, c.info["min_hamming"])
            assert (np.abs(c.v[:, :, :c.n_tok]) >= 2.0 ** -4).all() and (np.abs(c.v[:, :, :c.n_tok]) < 4).all()
            if c.npad > c.n_tok:
                assert (np.abs(c.v[:, :, c.n_tok:]) == 16384).all() and np.isnan(c.k[:, :, c.n_tok + 1:]).all()
                assert np.isfinite(c.k[:, :, c.n_tok]).all()
            if c.kernel == "causal":
                assert (c.info["pi"] <= np.arange(c.n_tok)).all()
        else:
            assert (c.v[:, :, :c.n_tok] >= 0).all() and (c.v[:, :, :c.n_tok] <= 15).all() and (c.v[:, :, c.n_tok:] == 4096).all()
        if c.family == "uniform":
            assert not c.q[:, :, :c.n_tok].any() and np.isnan(c.k[:, :, c.n_tok:]).all()
        if c.family in ("pow2", "nat8"):
            assert np.isfinite(c.k).all() and np.abs(c.k).max() <= (1600 if c.family == "nat8" else 200)
            assert (c.q[:, :, :c.n_tok].sum(-1) == 1).all() and (np.abs(c.q[:, :, :c.n_tok]).sum(-1) == 1).all()
            if c.family == "nat8":
                assert not (c.k % 8).any()
    assert least_ham >= 8 and worst_dev < 2.0 ** -20


def test_select_layout_places_heads_and_transposes_v():
    c = ac.select_case("dino", 2, 2, 64, 17, 0, False)
    qk, vt = ac.pack_qk_vt(c)
    f = ac.bits_to_f64
    assert np.array_equal(f(qk[1 * 32 + 5, 64:128]), c.q[1, 1, 5]) and np.array_equal(f(qk[0 * 32 + 16, 128:192]), c.k[0, 0, 16])
    assert np.array_equal(f(vt[1, 0, 7, :]), c.v[1, 0, :, 7])
    c = ac.select_case("hd", 2, 2, 104, 17, 0)
    qkv = ac.pack_qkv(c)
    assert np.array_equal(f(qkv[1, 3, 104:208]), c.q[1, 1, 3]) and np.array_equal(f(qkv[0, 4, 208:312]), c.k[0, 0, 4])
    assert np.array_equal(f(qkv[1, 16, 416 + 104:]), c.v[1, 1, 16])
    assert np.array_equal(ac.expected_rows(c)[1, 3, 104:], c.expected[1, 1, 3])


def test_pad_variants_change_only_pad_rows():
    base = ac.pow2_case("dino", 1, 3, 64, 65, 0)
    for pk in ("nan", "inf", "zero"):
        for pv in ("default", "zero"):
            c = ac.pow2_case("dino", 1, 3, 64, 65, 0, pk, pv)
            for a, b in ((c.q, base.q), (c.k, base.k), (c.v, base.v)):
                assert np.array_equal(a[:, :, :65], b[:, :, :65])
            assert np.array_equal(c.expected, base.expected)
            assert (np.isnan(c.k[:, :, 65:]).all(), np.isinf(c.k[:, :, 65:]).all(), not c.k[:, :, 65:].any()) == (pk == "nan", pk == "inf", pk == "zero")
            assert (not c.v[:, :, 65:].any()) == (pv == "zero")


# ---- references against exact arithmetic ----------------------------------------------------------------------------------------------


def _exact_pow2(case, b, h, t, d):
    L = [int(x) for x in case.info["logits"][b, h, t]]
    keys = range(t + 1) if case.causal else range(case.n_tok)
    lo = min(L[j] for j in keys)
    w = {j: 2 ** (L[j] - lo) for j in keys}
    return Fraction(sum(w[j] * int(case.v[b, h, j, d]) for j in keys), sum(w.values()))


@pytest.mark.parametrize("kernel,B,H,hd,n", [("dino", 1, 3, 64, 97), ("causal", 2, 2, 8, 17)])
def test_pow2_reference_is_the_exact_rational(kernel, B, H, hd, n):
    c = ac.pow2_case(kernel, B, H, hd, n, 0)
    for b in range(B):
        for h in range(H):
            for t in range(n):
                # the logits recorded per query are the q.k products of the arrays the kernel reads
                assert np.array_equal(c.k[b, h, :n].astype(np.float64) @ c.q[b, h, t].astype(np.float64), c.info["logits"][b, h, t])
                for d in range(0, hd, 5):
                    exact = _exact_pow2(c, b, h, t, d)
                    assert abs(Fraction(float(c.expected[b, h, t, d])) - exact) <= exact * Fraction(1, 2 ** 44)


@pytest.mark.parametrize("kernel,B,H,hd,n", [("dino", 1, 3, 64, 97), ("causal", 2, 2, 8, 17)])
def test_uniform_reference_is_the_exact_mean(kernel, B, H, hd, n):
    c = ac.uniform_case(kernel, B, H, hd, n, 0)
    for b in range(B):
        for h in range(H):
            for t in range(n):
                keys = range(t + 1) if c.causal else range(n)
                for d in range(hd):
                    exact = Fraction(sum(int(c.v[b, h, j, d]) for j in keys), len(keys))
                    assert abs(Fraction(float(c.expected[b, h, t, d])) - exact) <= exact * Fraction(1, 2 ** 50)


def test_nat8_reference_matches_integer_nats():
    c = ac.nat8_case(1, 3, 97, 0)
    b, h = 0, 1
    for t in (0, 17, 40, 96):
        nats = (c.k[b, h, :97].astype(np.float64) @ c.q[b, h, t].astype(np.float64)) / 8
        assert np.array_equal(nats, np.round(nats))
        w = np.exp(nats - nats.max())
        assert np.allclose((w[:, None] * c.v[b, h, :97]).sum(0) / w.sum(), c.expected[b, h, t], rtol=1e-12, atol=0)


# ---- the neighbour rule -----------------------------------------------------------------------------------------------------------------


def test_bf16_helpers():
    # ties go to the even mantissa: 1 + 2^-8 -> 1, 1 + 3 * 2^-8 -> 1 + 2^-6
    assert ac.bf16_round(np.float32([1 + 2.0 ** -8]))[0] == 1.0 and ac.bf16_round(np.float32([1 + 3 * 2.0 ** -8]))[0] == 1 + 2.0 ** -6
    assert ac.bf16_round(np.float32([1 + 2.0 ** -8 + 2.0 ** -20]))[0] == 1 + 2.0 ** -7
    assert ac.bf16_exact(np.float32([0.0, 255.0, 1336.0, -1200.0, 16384.0, np.nan, np.inf])) and not ac.bf16_exact(np.float32([257.0]))
    assert list(ac.bf16_bits(np.float32([1.0, -2.0, np.nan, np.inf]))) == [0x3F80, 0xC000, 0x7FC0, 0x7F80]
    assert list(ac.bits_to_f64(np.uint16([0x3F80, 0xC000, 0x4049]))) == [1.0, -2.0, 3.140625]
    assert list(ac.ulp_bf16([1.0, 1.99, 2.0, 0.75, 0.0, -3.0, 2.0 ** -100])) == [2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 0.0, 2.0 ** -6, 2.0 ** -107]


def test_bf16_neighbour_rule():
    nb = ac.bf16_neighbour
    u = 2.0 ** -7
    # a tie: both neighbours pass, the next ones out do not
    tie = 1.5 + u / 2
    assert list(nb([1.5, 1.5 + u, 1.5 - u, 1.5 + 2 * u], [tie] * 4)) == [True, True, False, False]
    # an ordinary value: its two bracketing bf16 numbers pass, two steps away fails
    x = 1 + 0.3 * u
    assert list(nb([1.0, 1 + u, 1 + 2 * u, 1 - u], [x] * 4)) == [True, True, False, False]
    # a power of two: one spacing of the binade ABOVE it on either side (two of the finer steps below), no more
    assert list(nb([2.0, 2 + 2 * u, 2 - 2 * u, 2 + 4 * u, 2 - 3 * u], [2.0] * 5)) == [True, True, True, False, False]
    # zero is exact, NaN never passes
    assert list(nb([0.0, -0.0, 2.0 ** -130, np.nan], [0.0, 0.0, 0.0, 1.0])) == [True, True, False, False]
    assert list(nb([0.0, 2.0 ** -100], [2.0 ** -120, 0.0], atol=ac.FLUSH_ATOL)) == [True, False]
    # the rule as check_output applies it
    c = ac.uniform_case("dino", 1, 1, 64, 15, 0)
    good = ac.bf16_round(c.expected.astype(np.float32)).astype(np.float64)
    assert ac.check_output(c, good).all()
    bad = good.copy()
    bad[0, 0, 3, 5] += 2 * ac.ulp_bf16(bad[0, 0, 3, 5]) if bad[0, 0, 3, 5] else 1.0
    assert not ac.check_output(c, bad)[0, 0, 3, 5] and ac.check_output(c, bad).sum() == bad.size - 1
    # one key too many or too few moves the uniform mean by more than the rule allows somewhere in every row
    v = c.v[0, 0, :15].astype(np.float64)
    short = np.broadcast_to(v[:14].mean(0), (15, 64))
    assert not ac.check_output(c, short[None, None]).all(axis=-1).any()
    s = ac.select_case("dino", 1, 1, 64, 15, 0, False)
    assert ac.check_output(s, s.expected).all() and not ac.check_output(s, s.expected * (1 + 2.0 ** -7)).any()
    n = ac.nat8_case(1, 1, 15, 0)
    assert ac.check_output(n, n.expected * (1 + 0.9 * ac.NAT8_RTOL)).all()
    nz = n.expected > 2.0 ** -90          # (below that the flush term of the rule takes over)
    assert not ac.check_output(n, n.expected * (1 + 1.1 * ac.NAT8_RTOL))[nz].any()
    assert ac.NAT8_RTOL == 2.0 ** -7 + 2.0 ** -8 + 2.0 ** -12
