"""The buffer contract of include/freepose_hip.h on the MI355X: every case of tests/_extent_cases.py — four calls of the entry, twice into
exact-fit tensors and twice embedded between 4 KiB guards under the fills 0xFF and 0x5A.  Nothing outside the documented extent of an
output is written (guards, stride gaps, bytes the header says are left alone), every documented byte is written, and nothing outside the
documented extent of an input reaches the result.  All inputs are valid and every store within 4 KiB of its buffer lands in a guard: no
case is meant to fault."""
import pytest
import torch

from tests import _extent_cases as ec

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("case", ec.CASES, ids=lambda c: c.name)
def test_extent(case):
    assert torch.cuda.is_available()
    torch.cuda.set_device(0)
    ec.run(case)


def test_torch_allocations_meet_the_placement():
    """the extent of an embedded region starts on a 256-byte boundary of device memory, a shifted one a single element behind a 16-byte one"""
    r = ec.Region("y", torch.bfloat16, (3, 5), ld=8, shift=1)
    P = ec.embed([r], 0x5A)["y"]
    assert P.buf.is_cuda and (P.buf.data_ptr() + ec.GUARD) % ec.ALIGN == 0 and P.ptr.value % 16 == 2
    assert bool((P.buf == 0x5A).all()) and P.buf.numel() == ec.GUARD + 2 + r.extent_bytes() + ec.GUARD
