"""The case table of the stream contract (tests/_stream_cases.py) against the header: every entry of include/freepose_hip.h that takes a
stream is named by a case or excused in EXCLUDED, and the two input sets of every case are what tests/test_gpu_streams.py relies on — the
same shapes and dtypes, finite, index-like inputs inside their ranges.  No GPU."""
import re
from pathlib import Path

import numpy as np
import pytest
import torch

from tests import _stream_cases as sc

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "freepose_hip.h"
N_STREAM_ENTRIES = 59                     # entries with a `void* stream` parameter today: a new one needs a case (or a reason) and this count


def stream_entries():
    text = re.sub(r"/\*.*?\*/", " ", HEADER.read_text(), flags=re.S)
    text = text[text.index('extern "C" {'):]
    out = []
    for name, params in re.findall(r"\b(fp_\w+)\s*\(([^;{]*?)\)\s*;", text, flags=re.S):
        if re.search(r"\bvoid\s*\*\s*stream\b", params):
            out.append(name)
    return out


def test_every_stream_entry_is_covered_or_excused():
    entries = stream_entries()
    assert len(entries) == len(set(entries)) == N_STREAM_ENTRIES, (len(entries), sorted(entries))
    named = {e for c in sc.CASES for e in c.entries}
    assert named <= set(entries), f"cases name entries the header does not have (or that take no stream): {sorted(named - set(entries))}"
    assert not (named & set(sc.EXCLUDED)), f"both covered and excluded: {sorted(named & set(sc.EXCLUDED))}"
    missing = sorted(set(entries) - named - set(sc.EXCLUDED))
    assert not missing, f"entries with a stream parameter that no case and no EXCLUDED reason names: {missing}"


def test_excluded_is_capped_and_every_reason_names_the_stream():
    assert len(sc.EXCLUDED) <= sc.MAX_EXCLUDED == 8
    assert set(sc.EXCLUDED) <= set(stream_entries())
    for entry, reason in sc.EXCLUDED.items():
        assert isinstance(reason, str) and "\n" not in reason and len(reason) > 20 and "stream" in reason, (entry, reason)
    assert isinstance(sc.DRAINS_DEVICE, dict) and set(sc.DRAINS_DEVICE) <= {c.name for c in sc.CASES}


def test_case_names_are_unique_and_the_controls_are_the_five():
    names = [c.name for c in sc.CASES]
    assert len(names) == len(set(names))
    assert sorted(sc.MUTANTS) == sorted(["l2_normalize", "gemm_tiny64", "attention_hd", "layernorm", "transpose"])
    for name in sc.MUTANTS:                                             # value-only entries: no check (no index-like input), every input late
        c = sc.by_name(name)
        assert c.check is None and c.late is None and not c.waits
    assert {"ffa_fused_B2", "vit_28x42_fused", "vit_28x42_unfused", "vit_native_fused", "vit_native_unfused", "clip_visual", "clip_text",
            "rasterize_tiled1"} == set(sc.HANDOVER)


@pytest.mark.parametrize("case", sc.CASES, ids=lambda c: c.name)
def test_inputs_of_both_sets(case):
    A, B = case.build("A"), case.build("B")
    assert A and list(A) == list(B)
    for k in A:
        a, b = A[k], B[k]
        assert isinstance(a, torch.Tensor) and not a.is_cuda and a.is_contiguous() and b.is_contiguous(), k
        assert a.shape == b.shape and a.dtype == b.dtype, (k, a.shape, b.shape, a.dtype, b.dtype)
        if a.is_floating_point():
            assert bool(torch.isfinite(a.float()).all()) and bool(torch.isfinite(b.float()).all()), f"{k}: a non-finite input"
    late = case.late if case.late is not None else tuple(A)
    assert late and set(late) <= set(A)
    assert any(not sc.same_bits(A[k], B[k]) for k in late), "the late inputs of A and B are the same: the case could not fail"
    for k in set(A) - set(late):                                        # what is not made late is the same in both sets
        assert sc.same_bits(A[k], B[k]), k
    if case.check is not None:
        case.check(A)
        case.check(B)
    if case.batches:
        for n in case.batches:
            An, Bn = case.build("A", n), case.build("B", n)
            assert all(An[k].shape == Bn[k].shape and An[k].dtype == Bn[k].dtype for k in An)
            assert any(An[k].shape[0] == n for k in An), (n, {k: tuple(v.shape) for k, v in An.items()})
            if case.check is not None:
                case.check(An)
                case.check(Bn)
        assert case.batches[1] != case.batches[0] and case.batches[1] > max(case.batches[0], case.batches[2]), "the side call must regrow the workspaces"


def test_gemm_shapes_are_the_tiers_they_claim():
    """one tiny64 and one small128 shape per entry, and the smallest M the planner splits (two launches); no big tier"""
    from tests import _gemm_cases as gc
    planned = [c for c in sc.CASES if c.plan]
    assert {c.name.rsplit("_", 1)[1] for c in planned} == {"tiny64", "small128", "split"}
    for c in planned:
        M, N, K, epi, ln_part, label = c.plan
        got, row0 = gc.plan(M, N, K, epi, ln_part=ln_part)
        assert got.startswith(label) and "big" not in got, (c.name, got)
        if label == "split_":
            assert 0 < row0 < M
            assert not any("split" in gc.plan(m, N, K, epi, ln_part=ln_part)[0] for m in range(1, M)), f"{c.name}: a smaller M splits too"
        else:
            assert row0 == 0
    assert (sc.SPLIT_M, sc.SPLIT_N) == (8193, 1024)


def test_same_bits_tells_bits_not_values():
    z = torch.zeros(3)
    assert sc.same_bits((z,), (z.clone(),)) and not sc.same_bits(z, -z) and not sc.same_bits(z, z.double()) and not sc.same_bits(z, torch.zeros(4))
    nan = torch.tensor([float("nan")])
    assert sc.same_bits(nan, nan.clone()) and sc.same_bits(None, None) and not sc.same_bits(None, z)
    assert np.array_equal(sc._rodrigues(np.zeros(3)), np.eye(3))
