"""The case table of the buffer contract (tests/_extent_cases.py) against the header, and the harness against host writers.  Every entry of
include/freepose_hip.h with a writable device pointer is named by a case or pinned to an existing guard-band test; every output region
has the shape and dtype the header text it quotes states; the masks tile their buffers and the FREE caps hold; and run() reports each of
five wrong numpy writers with the right region and byte offset, and passes the correct one.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _extent_cases as ec
from tests import _stream_cases as sc

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "freepose_hip.h"
N_WRITABLE_ENTRIES = 54                   # entries with a non-const `d_*` pointer parameter today: a new one needs a case (or a pin) and this count


def writable_entries():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    text = text[text.index('extern "C" {'):]
    out = []
    for name, params in re.findall(r"\b(fp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        for p in (q.strip() for q in params.split(",")):
            if re.search(r"\*\s*d_\w+$", p) and not p.startswith("const"):
                out.append(name)
                break
    return out


# ---- header against table ------------------------------------------------------------------------------------------------------------------------
def test_every_writable_entry_has_a_case_or_a_pin():
    entries = writable_entries()
    assert len(entries) == len(set(entries)) == N_WRITABLE_ENTRIES, (len(entries), sorted(entries))
    named = {e for c in ec.CASES for e in c.entries}
    assert named <= set(entries), f"cases name entries the header does not have (or that write no device buffer): {sorted(named - set(entries))}"
    assert not (named & set(ec.PINNED_ELSEWHERE)), f"both covered and pinned elsewhere: {sorted(named & set(ec.PINNED_ELSEWHERE))}"
    missing = sorted(set(entries) - named - set(ec.PINNED_ELSEWHERE))
    assert not missing, f"entries with a writable device pointer that no case and no pin names: {missing}"


def test_pins_are_capped_and_name_existing_tests():
    assert len(ec.PINNED_ELSEWHERE) <= ec.MAX_PINNED == 16
    assert set(ec.PINNED_ELSEWHERE) <= set(writable_entries())
    for entry, where in ec.PINNED_ELSEWHERE.items():
        path, _, test = where.partition("::")
        assert path.startswith("tests/test_gpu_") and test.startswith("test_"), (entry, where)
        text = (ROOT / path).read_text()
        assert re.search(rf"^def {re.escape(test)}\(", text, flags=re.M), f"{entry}: {where} does not exist"
        assert re.search(r"guard|GUARD", text) and re.search(r"0xFF|== -1|\b-1\b", text), f"{entry}: {path} has no pre-filled output with guards"


def test_case_names_are_unique_and_inputs_come_from_the_stream_table():
    names = [c.name for c in ec.CASES]
    assert len(names) == len(set(names))
    for c in ec.CASES:
        if c.wrapper:
            stream = sc.by_name(c.wrapper[0])
            assert set(c.entries) <= set(stream.entries), (c.name, c.entries, stream.entries)
            A, x = stream.build("A"), c.inputs()
            if c.name == "pts_diameter":                                 # the clouds back to back, as the wrapper hands them to the entry
                assert sc.same_bits(x["pts"], torch.cat(list(A.values())))
            else:
                assert sc.same_bits(tuple(x.get(k) for k in A), tuple(A.values())), f"{c.name}: compared with the wrapper on other inputs than set A"


def test_the_three_alignment_placements():
    assert set(ec.MISALIGNED) == {"fp_gt_visibility", "fp_ffa", "fp_rerank_views"}
    shifted = {}
    for c in ec.CASES:
        for r in c.regions(c.inputs()):
            if r.shift:
                assert r.shift == 1, (c.name, r.name)
                shifted.setdefault(c.name, []).append(r.name)
    assert set(shifted) == set(ec.MISALIGNED.values()), f"misaligned placements are for the three launchers that test alignment only: {shifted}"
    for entry, name in ec.MISALIGNED.items():
        assert ec.by_name(name).entries == (entry,)


# ---- every case's regions and masks --------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def header():
    return ec.header_text(HEADER)


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.name)
def test_regions_and_masks(case, header):
    x = case.inputs()
    regions = case.regions(x)
    assert len({r.name for r in regions}) == len(regions)
    written = [r for r in regions if r.role != "in"]
    assert written, "a case without an output"
    for r in regions:
        if r.role == "in":
            assert r.quote == () and r.data is not None
            if r.data.is_floating_point():
                assert bool(torch.isfinite(r.data.float()).all()), r.name
    for r in written:                                                    # shape and dtype as the quoted header text states them
        assert r.quote, f"{r.name}: an output quotes the header text that states its shape"
        for q in r.quote:
            assert re.sub(r"\s+", " ", q) in header, f"{r.name}: the header does not say {q!r}"
        dtype, shape = ec.parse_quote(r.quote, r.dims)
        assert shape == r.shape, (r.name, shape, r.shape)
        assert dtype == r.dtype or (dtype is None and r.dtype == torch.uint8 and "bytes" in r.quote[0]), (r.name, dtype, r.dtype)
        if r.ld is not None:
            assert r.ld > r.cols, f"{r.name}: a leading dimension equal to the row length has no gap to guard"
    elem = ec.element_masks(case, x, regions, case.host_example)
    free_regions = 0
    for r in written:
        for tight in (True, False):
            P = ec.embed([r], 0x5A, "cpu", tight)[r.name]
            m = ec.byte_mask(r, elem.get(r.name), P)
            assert m.shape == (P.buf.numel(),) and set(np.unique(m)) <= {ec.MUST, ec.NEVER, ec.FREE}      # MUST | NEVER | FREE tiles the buffer
            inside = int((m != ec.NEVER).sum()) + int((np.asarray(elem.get(r.name, 1)) == ec.NEVER).sum()) * r.itemsize
            assert inside == r.rows * r.cols * r.itemsize
            if not tight:
                assert P.start == ec.GUARD + r.shift * r.itemsize and P.buf.numel() == P.start + r.extent_bytes() + ec.GUARD
                assert (m[:P.start] == ec.NEVER).all() and (m[P.start + r.extent_bytes():] == ec.NEVER).all()
                assert (P.buf.data_ptr() + ec.GUARD) % ec.ALIGN == 0 and (P.buf.data_ptr() + P.start) % 16 == r.shift * r.itemsize
                if r.ld is not None:
                    gaps = m[P.start:P.start + r.extent_bytes()].reshape(-1)[:(r.rows - 1) * r.ld * r.itemsize].reshape(r.rows - 1, r.ld * r.itemsize)
                    assert (gaps[:, r.cols * r.itemsize:] == ec.NEVER).all(), "stride gaps count as guard"
        free = int((np.asarray(elem.get(r.name, 1)) == ec.FREE).sum())
        if free:
            free_regions += 1
            assert 2 * free <= r.rows * r.cols, f"{r.name}: FREE covers more than half of the region"
            assert r.name in case.free and re.sub(r"\s+", " ", case.free[r.name]) in header, f"{r.name}: FREE bytes need a sentence of the header"
        assert (np.asarray(elem.get(r.name, 1)) == ec.MUST).any(), f"{r.name}: nothing of the region must be written"
    assert set(case.free) == {r.name for r in written if (np.asarray(elem.get(r.name, 1)) == ec.FREE).any()}
    assert bool(case.free) == bool(free_regions)


def test_free_caps():
    assert sum(1 for c in ec.CASES if c.free) <= ec.MAX_FREE_CASES == 6


def test_index_like_inputs_are_the_ones_the_stream_table_checks():
    """the tables, ranges, ids and counts — the inputs of the stream cases that have a `check` — have zero guards; float data has the fill"""
    for c in ec.CASES:
        regions = c.regions(c.inputs())
        marked = {r.name for r in regions if r.index_like}
        if c.wrapper and sc.by_name(c.wrapper[0]).check is not None and c.name != "depthmap_scales":      # (its check is of the masks: data, not indices)
            assert marked, f"{c.name}: the stream table checks its index-like inputs, the case marks none"
        for r in regions:
            if r.index_like:
                assert r.role == "in"
                P = ec.embed([r], 0xFF, "cpu")[r.name]
                assert (P.buf[:P.start] == 0).all() and (P.buf[P.start + r.extent_bytes():] == 0).all()
            elif r.role == "in":
                P = ec.embed([r], 0xFF, "cpu")[r.name]
                assert (P.buf[:P.start] == 0xFF).all() and (P.buf[P.start + r.extent_bytes():] == 0xFF).all()


# ---- the harness can fail: numpy writers on host buffers -------------------------------------------------------------------------------------------
ROWS, COLS, LD = 3, 5, 8


def _toy(x_last=1.5):
    def inputs():
        x = torch.arange(1, ROWS * COLS + 1, dtype=torch.float32).reshape(ROWS, COLS) / 4
        x[-1, -1] = x_last
        return dict(x=x)

    def regions(x):
        return ec._ins(x, x=dict(ld=LD)) + [ec.Region("y", torch.float32, (ROWS, COLS), ld=LD)]
    return ec.ExtentCase("toy", ("toy",), inputs, regions, None)


def _correct(P, x):
    P["y"].typed().copy_(2 * P["x"].typed())


def _past_the_end(P, x):
    _correct(P, x)
    e = P["y"].element((ROWS - 1) * P["y"].ld + COLS)
    if e is not None:
        e[0] = 7.0


def _into_the_gap(P, x):
    _correct(P, x)
    if P["y"].ld > COLS:
        P["y"].element(1 * P["y"].ld + COLS)[0] = 7.0


def _skips_the_last(P, x):
    y = P["y"].typed()
    for r in range(ROWS):
        n = COLS - 1 if r == ROWS - 1 else COLS
        y[r, :n] = 2 * P["x"].typed()[r, :n]


def _reads_the_guard(P, x):
    _correct(P, x)
    g = P["x"].element((ROWS - 1) * P["x"].ld + COLS)                    # the first guard element behind the input
    if g is not None:
        P["y"].typed()[0, 0] += g[0]


def test_a_correct_writer_passes():
    assert ec.run(_toy(), "cpu", _correct) is None


@pytest.mark.parametrize("writer, x_last, kind, region, row, col", [
    (_past_the_end, 1.5, "never", "y", ROWS - 1, COLS),                  # one element past the extent
    (_into_the_gap, 1.5, "never", "y", 1, COLS),                         # into a stride gap
    (_skips_the_last, 1.5, "unwritten", "y", ROWS - 1, COLS - 1),        # the last element of the last row
    (_skips_the_last, 0.0, "unwritten", "y", ROWS - 1, COLS - 1),        # ... whose correct value is 0: the exact-fit run is right by accident
    (_reads_the_guard, 1.5, "unwritten", "y", 0, 0),                     # the first guard element of an input added to the result
], ids=["past_the_end", "stride_gap", "skips_last", "skips_last_correct_value_zero", "reads_input_guard"])
def test_a_wrong_writer_is_reported(writer, x_last, kind, region, row, col):
    with pytest.raises(ec.ExtentError) as e:
        ec.run(_toy(x_last), "cpu", writer)
    err = e.value
    assert (err.kind, err.region, err.row, err.col) == (kind, region, row, col), str(err)
    assert err.offset == (row * LD + col) * 4 and f"byte offset {err.offset}" in str(err) and f"region {region}" in str(err), str(err)


def test_the_zero_valued_skip_is_caught_by_the_two_fills_alone():
    """the skipped element's correct value is 0 and the exact-fit output is zero-filled: the two exact-fit runs agree and hold the right
    bits, one pre-filled run would too under a zero fill — only the disagreement of the 0xFF and 0x5A runs shows the store is missing"""
    case = _toy(0.0)
    x = case.inputs()
    P = ec.embed(case.regions(x), 0, "cpu", tight=True)
    _skips_the_last(P, x)
    assert torch.equal(P["y"].typed(), 2 * x["x"])


def test_a_guard_read_under_a_finite_fill_is_a_leak():
    """with one fill only (0x5A twice) the guard read gives equal embedded runs; it is the comparison with the exact-fit run that reports it"""
    saved = ec.FILLS
    ec.FILLS = (0x5A, 0x5A)
    try:
        with pytest.raises(ec.ExtentError) as e:
            ec.run(_toy(), "cpu", _reads_the_guard)
    finally:
        ec.FILLS = saved
    assert (e.value.kind, e.value.region, e.value.offset) == ("leak", "y", 0)


def test_an_unrepeatable_entry_is_its_own_finding():
    calls = []

    def drifting(P, x):
        _correct(P, x)
        calls.append(1)
        P["y"].typed()[1, 2] += len(calls)
    with pytest.raises(ec.NotRepeatable):
        ec.run(_toy(), "cpu", drifting)


def test_a_written_input_is_reported():
    def clobbers(P, x):
        _correct(P, x)
        P["x"].typed()[2, 1] = 0.0
    with pytest.raises(ec.ExtentError) as e:
        ec.run(_toy(), "cpu", clobbers)
    assert (e.value.kind, e.value.region, e.value.row, e.value.col) == ("never", "x", 2, 1)
