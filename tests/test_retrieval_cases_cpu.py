"""The planted retrieval cases of tests/_retrieval_cases.py, checked without a GPU: the numpy references equal the C oracle bit for bit (two
references with the same bug would have to share it across numpy's lexsort and C's qsort), and every case reaches the kernel branch its id
claims according to the mirror of the dispatch predicates — a case that drifts off its branch after a later edit fails here, not silently
on the GPU.  Run with -s to see the branch assigned to every case id."""
import numpy as np
import pytest

from tests import _retrieval_cases as rc

NCU = 256      # the MI355X; a GPU test reads the count from the device


@pytest.fixture(scope="module")
def banks():
    return {b: make() for b, make in rc.SELECT_BANKS.items()}


def test_key_mapping_round_trips_and_orders():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    finite = bits[((bits & 0x7F80) != 0x7F80) | ((bits & 0x7F) == 0)]         # drop NaN
    finite = finite[finite != 0x8000]                                          # and -0.0
    keys = rc.key16(finite)
    assert np.array_equal(rc.key_to_bits(keys), finite)
    order = np.argsort(keys.astype(np.int64), kind="stable")
    assert (np.diff(rc.bits_f32(finite)[order].astype(np.float64)) > 0).all(), "key order is score order, strictly"
    assert rc.key16([0xFF80])[0] == rc.K_NINF and rc.key16([0x7F80])[0] == rc.K_PINF and rc.key16([0])[0] == rc.K_ZERO


@pytest.mark.parametrize("bank_id", list(rc.SELECT_BANKS))
def test_planted_topk_ref_equals_oracle(banks, bank_id):
    """for each of the three planted queries: the scores the planting predicts are the oracle's, and topk_ref is the oracle's top-k"""
    from oracle import fp_oracle as fo
    bits = banks[bank_id]
    N = len(bits)
    assert not (((bits & 0x7F80) == 0x7F80) & ((bits & 0x7F) != 0)).any() and not (bits == 0x8000).any(), "NaN and -0.0 stay out"
    k = min(N, rc.KMAX)
    bank, q = rc.planted_bank(bits), rc.planted_queries()
    s_o, i_o = fo.bank_topk(bank, q, k, idx_offset=12345)
    for qi, qb in enumerate((rc.Q_E0, rc.Q_NEG, rc.Q_TWO)):
        sc = rc.planted_scores(bits, qb)
        if qi == 0:
            assert np.array_equal(sc, bits)
        s_r, i_r = rc.topk_ref(sc, k, 12345)
        assert np.array_equal(i_r, i_o[qi]) and np.array_equal(s_r.view(np.uint32), s_o[qi].view(np.uint32)), (bank_id, qi)


def test_every_select_case_lands_on_its_branch(banks):
    seen, hi_exact, lo_exact = set(), set(), set()
    for cid, b, k, off, claim in rc.SELECT_CASES:
        sp = rc.select_path(rc.key16(banks[b]), k)
        print(f"{cid:32s} -> {sp['path']:18s} " + " ".join(f"{n}={v}" for n, v in sp.items() if n != "path" and v is not None))
        assert sp["path"] == claim, (cid, sp)
        assert off + len(banks[b]) - 1 <= 2 ** 31 - 1
        seen.add(sp["path"])
        if sp["path"].startswith("hist"):
            tied_end = sp["neq"] > 1 and sp["ngt"] + sp["neq"] == k      # a plateau that ends exactly at k
            if sp["hi_exact"] and tied_end:
                hi_exact.add(sp["path"])
            if sp["lo_exact"] and not sp["hi_exact"] and tied_end:
                lo_exact.add(sp["path"])
        if cid in rc.PLATEAU_SEARCH_CASES:
            assert 0 < sp["L"] < sp["T"] < sp["G"] and sp["iters"] >= 3 and sp["cut_inside"], (cid, sp)
    assert seen == {"reg-fast", "reg-count-rank", "reg-count-bitonic", "hist-lds", "hist-global"}
    assert hi_exact == lo_exact == {"hist-lds", "hist-global"}, "`c + hist[b] == k` exactly, at either byte's scan, in both histogram kernels"
    assert {(c[2], c[4]) for c in rc.SELECT_CASES if c[0] in rc.PLATEAU_SEARCH_CASES} >= {
        (100, "reg-count-rank"), (257, "reg-count-bitonic"), (500, "reg-count-bitonic"), (1024, "reg-count-bitonic")}
    m0, m1 = (rc.select_path(rc.key16(banks[b]), 100) for b in ("m1024", "m1025"))
    assert (m0["M"], m0["path"], m1["M"], m1["path"]) == (rc.KMAX, "reg-fast", rc.KMAX + 1, "reg-count-rank")
    p4 = rc.select_path(rc.key16(banks["plat40000"]), 1024)
    assert p4["neq"] >= 2 ** 15 and p4["ngt"] > 0
    assert rc.select_path(rc.key16(banks["plat70000"]), 100)["neq"] > 65535
    assert rc.select_path(rc.key16(banks["n100"]), 100)["L"] == 0
    sizes = {len(banks[c[1]]) for c in rc.SELECT_CASES}
    assert {1, 7, 8, 9, 47, 48, 49, 100, 1024, 49151, 49152, 49153, 60001, 65536, 65537, 106501} <= sizes


def test_scan_classes_at_256_cus():
    for rows in rc.SCAN_ROWS:
        N = rc.scan_n_for(rows, NCU)
        base, rem, nwave = rc.scan_rows_per_wave(N, NCU)
        print(f"scan rows/wave {rows:2d}: N = {N:6d}  base_rows {base} rem {rem} nwave {nwave}  in-loop fetches {rc.scan_inloop_fetches(base)}"
              f" / {rc.scan_inloop_fetches(base + 1)}")
        assert base == rows and (rem != 0 or rows == 0) and N <= 180000
    for rows in rc.SCAN_ROWS_D1536:                       # three 16-byte loads per lane and row; one query keeps the oracle call small
        N = rc.scan_n_for(rows, NCU)
        print(f"scan rows/wave {rows:2d} at D = 1536: N = {N}, {N * 1536 * 2 / 2 ** 20:.0f} MiB")
        assert rc.scan_rows_per_wave(N, NCU)[0] == rows and rc.scan_form(1536) == (3, True) and N * 1536 * 1 <= 2e8
    assert max(rc.scan_n_for(r, NCU) for r in rc.SCAN_ROWS) * 64 * 5 <= 2e8, "the long runs use D <= 64 with five queries"
    assert rc.scan_rows_per_wave(3, NCU) == (0, 3, 4), "N = 3: one workgroup, three waves with one row and an idle one"
    assert [rc.scan_inloop_fetches(r) for r in (9, 12, 13, 20, 21, 22)] == [0, 0, 1, 1, 2, 2]
    assert rc.scan_rows_per_wave(46037, NCU)[0] == 8 and rc.scan_rows_per_wave(8000, NCU)[0] <= 1, "the workload's banks never get there"
    assert {rc.scan_form(D) for D in rc.SCAN_D} == {(1, False), (1, True), (2, False), (2, True), (3, False), (3, True)}
    assert [rc.scan_passes(Q) for Q in rc.SCAN_Q] == [[1], [1, 1, 1], [4], [4, 1], [4, 4], [4, 4, 1]]


def test_normed_scorer_wave_ownership():
    owned = set()
    for cid, T, P, owns in rc.NORMED_CASES:
        TS, got, idle = rc.normed_ts(T, P)
        print(f"{cid:12s} T={T} P={P}: TS={TS} templates per wave {got} waves past P {idle}")
        assert got == owns, cid
        owned |= set(got)
    assert set(range(1, 8)) <= owned
    assert rc.normed_ts(5, 3)[0] == 5 and rc.normed_ts(600, 7)[0] == 586 and rc.normed_ts(19, 1023)[2] > 0
    for _, T, P in rc.RAW_CASES:
        assert T * P > 16384 and (T * P) % 4 != 0
    assert max(T * P for _, T, P, *_ in rc.NORMED_CASES + rc.RAW_CASES) * max(rc.TEMPLATE_D) <= 2e8


def test_div_sweep_reference_equals_oracle_and_hits_the_fallback_window():
    from oracle import fp_oracle as fo
    rows = np.concatenate([rc.div_sweep(), rc.div_small_group()])
    want, q, n = rc.div_ref(rows)
    onehot = np.zeros((1, 8), np.uint16)
    onehot[0, 0] = 0x3F80
    got = fo.template_score(rows.reshape(-1, 1, 8), onehot)
    assert np.array_equal(fo.to_bf16_bits(got), rc.div_observed(want)) and np.array_equal(got.view(np.uint32) & 0xFFFF, np.zeros(len(rows), np.uint32))
    main = slice(0, rc.DIV_MAIN_ROWS)
    assert len(np.unique(rows[main, 0])) == 4 * 2 * 128 and len(np.unique(rc.bf16_rne(n[main]) & 0x7F)) == 128
    lanes = rc.div_fallback_lanes(q)
    print(f"div sweep: {len(rows)} rows, {int(lanes.sum())} quotients within 4 of a bf16 midpoint ({int(lanes[main].sum())} of them in the "
          f"normal-range sweep), {int((np.abs(q) < 2.0 ** -126).sum())} denormal quotients")
    assert lanes.sum() >= 1000
    assert lanes[main].sum() == 0, "a ratio of two 8-bit mantissas stays 2^-17 away from every bf16 midpoint"
    small = q[-12:]
    assert (np.abs(small[:-1]) < 2.0 ** -126).all() and (small[:-1] != 0).all() and small[-1] == 0 and n[-1] == np.float32(1e-12)


@pytest.mark.parametrize("C", rc.MERGE_C)
def test_merge_ref_equals_oracle(C):
    from oracle import fp_oracle as fo
    cs, ci = rc.merge_case(C)
    assert not np.isnan(cs).any() and (cs[4].view(np.uint32) & 0xFFFF).any(), "row 4 is not bf16-valued"
    for k in sorted({1, C, min(C, 1024)}):
        s_o, i_o = fo.topk_merge(cs, ci, k)
        for q in range(rc.MERGE_Q):
            s_r, i_r = rc.merge_ref(cs[q], ci[q], k)
            assert np.array_equal(i_r, i_o[q]) and np.array_equal(s_r.view(np.uint32), s_o[q].view(np.uint32)), (C, k, q)


def test_rerank_case_plants_its_best_views_past_the_clamp():
    from oracle import fp_oracle as fo
    views, off, cand, q = rc.rerank_case(8)
    assert list(np.diff(off)) == list(rc.RERANK_NV) and (cand[0] == 3).sum() == 2
    mesh = rc.RERANK_NV.index(1030)
    for k in rc.RERANK_K:
        o = fo.rerank_views(views, off, cand, q, k)
        assert np.array_equal(rc.rerank_ref8(views, off, cand, q, k).view(np.uint32), o.view(np.uint32)), k
        assert o[0, rc.RERANK_NV.index(0)] == np.float32(-3.0e38)
        counted_all = rc.rerank_ref8(views, off, cand, q, k, maxv=10 ** 6)
        assert counted_all[0, mesh] > o[0, mesh], "the views past row 1024 are the best ones: counting them would show"
