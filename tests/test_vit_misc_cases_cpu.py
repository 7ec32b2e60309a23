"""The references of tests/_vit_misc_cases.py are right and its bounds have teeth (no GPU): the float64 references equal torch's float64
operators, the record encoding round-trips, every restatement stays inside its stored E_case (so inside a quarter of its bound), and every
listed mutant of a restatement is rejected by the bound on at least one committed case."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

from tests import _vit_misc_cases as vc


def _rejected(got_bits, ref, E, S):
    """the bf16 bits break the bound somewhere (a NaN breaks it)"""
    err = np.abs(vc.bits_f32(got_bits).astype(np.float64) - ref)
    return bool((~(err <= vc.bound_bf16(ref, E, S))).any())


def _rejected_f32(got, ref, E, S):
    return bool((~(np.abs(np.asarray(got, dtype=np.float64) - ref) <= vc.bound_f32(ref, E, S))).any())


# ---- the references are right ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", vc.POSEMBED_CASES, ids=lambda c: c.name)
def test_posembed_reference_is_torch_float64(case):
    x = vc.posembed_input(case)
    ref, S = vc.posembed_ref64(x, case.G, case.gh, case.gw)
    t = torch.from_numpy(vc.bits_f32(x).astype(np.float64).reshape(1, case.G, case.G, case.D)).permute(0, 3, 1, 2)
    want = F.interpolate(t, size=(case.gh, case.gw), mode="bicubic", antialias=True).permute(0, 2, 3, 1).reshape(case.gh * case.gw, case.D)
    assert np.abs(ref - want.numpy()).max() <= 1e-12
    assert (S >= np.abs(ref) - 1e-12).all()


@pytest.mark.parametrize("case", vc.LN_CASES[:-1], ids=lambda c: c.name)
def test_layernorm_reference_is_torch_float64(case):
    x, g, b = vc.ln_inputs(case)
    ref, S = vc.ln_ref64(x, g, b)
    tx, tg, tb = (torch.from_numpy(vc.bits_f32(t).astype(np.float64)) for t in (x, g, b))
    want = F.layer_norm(tx, (case.D,), tg, tb, eps=float(np.float32(vc.EPS))).numpy()
    assert np.abs(ref - want).max() <= 1e-12 * max(1.0, np.abs(want).max())
    assert (S >= np.abs(ref) * (1 - 1e-12)).all()


def test_bf16_helpers_are_torch():
    x = np.random.default_rng(1).standard_normal(4096).astype(np.float32) * np.float32(3)
    x[:4] = [0.0, -0.0, 1.00390625, 1.01171875]                               # two ties: to even, down and up
    want = torch.from_numpy(x).to(torch.bfloat16).view(torch.int16).numpy().view(np.uint16)
    assert np.array_equal(vc.bf16_bits(x), want)
    assert np.array_equal(vc.bits_f32(want), torch.from_numpy(x).to(torch.bfloat16).float().numpy())
    assert vc.half_ulp_bf16(1.0) == 2.0 ** -8 and vc.half_ulp_bf16(1.99) == 2.0 ** -8 and vc.half_ulp_bf16(-0.75) == 2.0 ** -9 and vc.half_ulp_bf16(0.0) == 0


def test_records_round_trip():
    rng = np.random.default_rng(2)
    mean = (rng.standard_normal(1000) * 10 ** rng.uniform(-3, 2, 1000)).astype(np.float32)
    sigma = (10 ** rng.uniform(-3, 2, 1000)).astype(np.float32)
    m, s = vc.decode_row_record(vc.row_record(mean, sigma))
    assert (np.abs(m - mean) <= 2.0 ** -16 * np.abs(mean)).all() and (np.abs(s - sigma) <= 2.0 ** -16 * sigma).all()
    bad = vc.row_record(mean, sigma)
    bad[3, 2] ^= 1
    with pytest.raises(AssertionError, match="duplicated"):
        vc.decode_row_record(bad)


def test_l2_restatement_is_the_oracle():
    """the stand-in for ops.l2_normalize without a device: the C oracle's l2norm_rows, bit for bit"""
    from freepose_amd import build
    from oracle import fp_oracle as fo
    build.build_oracle(verbose=False)
    for case in (c for c in vc.LN_CASES if c.D <= vc.LN_L2_MAX_D and c.rows == 5 and c.regime != "const"):
        x, g, b = vc.ln_inputs(case)
        y = vc.bf16_bits(vc.ln_restate(x, g, b))
        assert np.array_equal(vc.l2_restate(y), np.asarray(fo.l2norm_rows(y)).view(np.uint16).reshape(y.shape)), case.name


# ---- the restatements stay inside their own bound ----------------------------------------------------------------------------------------------
def test_e_table_is_complete():
    assert sorted(vc.E_CASE) == sorted(vc.e_names()) and sorted(vc.POS_MISMATCH_MEASURED) == sorted(c.name for c in vc.POSEMBED_CASES)


@pytest.mark.parametrize("name", vc.e_names())
def test_restatement_inside_its_own_bound(name):
    """|restatement - ref64| <= E_case S, a quarter of the bound's 4 E_case S"""
    assert vc.measured_e(name) <= vc.E_CASE[name], f"{name}: the restatement left its stored E_case; measure_e() prints the table anew"


@pytest.mark.parametrize("case", vc.POSEMBED_CASES, ids=lambda c: c.name)
def test_posembed_restatement_is_torch_float32_path(case):
    x = vc.posembed_input(case)
    mine = vc.bf16_bits(vc.posembed_restate(x, case.G, case.gh, case.gw))
    share = float((mine != vc.posembed_torch_f32_bits(x, case.G, case.gh, case.gw)).mean())
    print(f"{case.name}: {share:.5%} of the restatement's elements differ in bits from torch's float32 path")
    assert share <= vc.POS_MISMATCH_CPU and share <= vc.POS_MISMATCH_MEASURED[case.name] + 1e-5
    if case.name == "pos_identity":
        assert np.array_equal(mine, x)


# ---- every listed mutant is rejected -------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def pos_refs():
    out = {}
    for c in vc.POSEMBED_CASES:
        x = vc.posembed_input(c)
        out[c.name] = (x,) + vc.posembed_ref64(x, c.G, c.gh, c.gw)
    return out


@pytest.mark.parametrize("mutant", sorted(vc.POSEMBED_MUTANTS))
def test_posembed_mutant_is_rejected(mutant, pos_refs):
    hits = []
    for c in vc.POSEMBED_CASES:
        x, ref, S = pos_refs[c.name]
        assert not _rejected(vc.bf16_bits(vc.posembed_restate(x, c.G, c.gh, c.gw)), ref, vc.E_CASE[c.name], S), c.name
        if _rejected(vc.bf16_bits(vc.posembed_restate(x, c.G, c.gh, c.gw, **vc.POSEMBED_MUTANTS[mutant])), ref, vc.E_CASE[c.name], S):
            hits.append(c.name)
    print(f"{mutant}: rejected on {hits}")
    assert hits


@pytest.mark.parametrize("mutant", vc.LN_MUTANTS[:4])
def test_layernorm_mutant_is_rejected(mutant):
    hits = []
    for c in vc.LN_CASES[:-1]:
        x, g, b = vc.ln_inputs(c)
        ref, S = vc.ln_ref64(x, g, b)
        assert not _rejected(vc.bf16_bits(vc.ln_restate(x, g, b)), ref, vc.E_CASE[c.name], S), c.name
        if _rejected(vc.bf16_bits(vc.ln_restate(x, g, b, mutant=mutant)), ref, vc.E_CASE[c.name], S):
            hits.append(c.name)
    print(f"{mutant}: rejected on {hits}")
    assert hits
    if mutant in ("eps_1e5", "eps_dropped"):
        assert any("lowvar" in h for h in hits)
    if mutant == "one_pass":
        assert any("offset" in h for h in hits)


def test_layernorm_const_rows_are_beta():
    for c in (c for c in vc.LN_CASES if c.regime == "const"):
        x, g, b = vc.ln_inputs(c)
        assert np.array_equal(vc.bf16_bits(vc.ln_restate(x, g, b)), np.broadcast_to(b, x.shape))


def test_l2_and_gather_mutants_are_rejected():
    """no tolerance on these two: the L2 form must give fp_l2_normalize's bits, the gather form the plain form's bits on the selected rows"""
    differs = 0
    for c in (c for c in vc.LN_CASES if c.D <= vc.LN_L2_MAX_D and c.rows == 5 and c.regime != "const"):
        x, g, b = vc.ln_inputs(c)
        y = vc.bf16_bits(vc.ln_restate(x, g, b))
        differs += int((vc.l2_restate(y) != vc.l2_restate(y, round_norm=False)).any())
    assert differs
    n = vc.GATHER_B * vc.GATHER_NPAD
    seen = np.zeros(n, dtype=int)
    for name, (rpb, stride, off) in vc.gather_forms().items():
        rows = vc.GATHER_B * rpb
        sel, shifted = vc.gather_rows(rows, rpb, stride, off), vc.gather_rows(rows, rpb, stride, off, off_by=1)
        assert sel.max() < n and len(set(sel)) == rows and not np.array_equal(sel, shifted), name
        seen[sel] += 1
    assert (seen == 1).all()                                                   # the three forms select every token row once: n_tok == npad here


@pytest.mark.parametrize("mutant", vc.TOKEN_MUTANTS)
def test_token_mutant_is_rejected(mutant):
    hits = []
    for c in vc.TOKEN_CASES:
        cls, pos0, reg = vc.token_inputs(c)
        want = vc.token_expected(c, cls, pos0, reg)
        n_tok, npad = vc.token_dims(c)
        assert want.shape == (c.B, npad, c.D) and (want[:, 1 + c.nreg:n_tok] == vc.TOKEN_PATTERN).all() and not want[:, n_tok:].any()
        if not np.array_equal(vc.token_expected(c, cls, pos0, reg, mutant), want):
            hits.append(c.name)
    assert hits
    assert vc.token_dims(vc.TOKEN_CASES[0]) == (261, 272) and vc.token_dims(vc.TOKEN_CASES[1]) == (16, 16)


@pytest.mark.parametrize("mutant", vc.FOLD_MUTANTS)
def test_fold_mutant_is_rejected(mutant):
    hits = []
    for c in vc.FOLD_CASES:
        W, g, be, bi = vc.fold_inputs(c)
        Wf, cs, bp = vc.fold_restate(W, g, be, bi, c.n_scaled, c.row_scale)
        refs = vc.fold_ref64(W, be, bi, Wf, c.n_scaled, c.row_scale)
        unscaled = np.arange(c.N) >= c.n_scaled
        assert np.array_equal(Wf[unscaled], vc.bf16_bits(vc.bits_f32(W) * vc.bits_f32(g))[unscaled])
        mWf, mcs, mbp = vc.fold_restate(W, g, be, bi, c.n_scaled, c.row_scale, mutant)
        for name, got, bad in (("colsum", cs, mcs), ("bprime", bp, mbp)):
            assert not _rejected_f32(got, *((refs[name][0], vc.E_CASE[f"{c.name}:{name}"], refs[name][1]))), (c.name, name)
        if (not np.array_equal(mWf, Wf) or _rejected_f32(mcs, refs["colsum"][0], vc.E_CASE[c.name + ":colsum"], refs["colsum"][1])
                or _rejected_f32(mbp, refs["bprime"][0], vc.E_CASE[c.name + ":bprime"], refs["bprime"][1])):
            hits.append(c.name)
    print(f"{mutant}: rejected on {hits}")
    assert hits


@pytest.mark.parametrize("mutant", vc.STAT_MUTANTS)
def test_stats_mutant_is_rejected(mutant):
    hits = []
    for c in vc.STAT_CASES[:-1] + vc.FIN_CASES:
        x = vc.stat_inputs(c)
        if isinstance(c, vc.StatCase):
            got, bad, refs = vc.row_stats_restate(x), vc.row_stats_restate(x, mutant=mutant), vc.row_stats_ref64(x)
        else:
            part = vc.partial_sums(x, c.pad)
            assert np.isnan(part[:, c.rows:]).all() and part.shape[1] == c.rows + c.pad
            got, bad, refs = vc.finalize_restate(part, c.rows), vc.finalize_restate(part, c.rows, mutant=mutant), vc.finalize_ref64(part, c.rows)
        for i, name in enumerate(("mean", "sigma", "rstd")):
            E = vc.E_CASE[f"{c.name}:{name}"]
            assert not _rejected_f32(got[i], refs[name][0], E, refs[name][1]), (c.name, name)
            if _rejected_f32(bad[i], refs[name][0], E, refs[name][1]):
                hits.append(f"{c.name}:{name}")
    print(f"{mutant}: rejected on {len(hits)} outputs")
    assert hits
    if mutant == "sigma_no_eps":
        assert any(h.startswith("rs_") for h in hits) and any(h.startswith("fin_") for h in hits)


def test_transpose_input_has_no_repeats_in_a_row():
    for rows, cols in vc.TRANSPOSE_CASES:
        x = vc.transpose_input(rows, cols)
        assert x.shape == (rows, cols) and (rows * cols < 3 or len(np.unique(x[:1].ravel()[:64])) == min(cols, 64))
