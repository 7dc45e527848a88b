"""-m gpu: `ops.image_metrics` and `ops.image_ssim` reproduce, BIT FOR BIT, the fp64 outputs recorded in tests/golden/ssim_bits.json on the cases of
tests/ssim_bits_cases.py.  The two entries share one tile body (csrc/ssim_shared.h), so the test that compares them with each other cannot see a change
both make; the fixture was written by tools/gen_ssim_bits.py from the library as it stood before the body was shared."""
import json
import os

import pytest
import torch

import ssim_bits_cases as SB
from selftoktokenizer_amd import ops

pytestmark = pytest.mark.gpu
GOLD = os.path.join(os.path.dirname(__file__), "golden", SB.FIXTURE)


@pytest.fixture(scope="module")
def want():
    with open(GOLD) as f:
        return json.load(f)


@pytest.fixture(scope="module")
def got():
    return SB.run(ops, torch, torch.device("cuda", 0))


@pytest.mark.parametrize("entry", ["image_metrics", "image_ssim"])
def test_the_recorded_bits(entry, want, got):
    cases = [c.name for c in (SB.metrics_cases() if entry == "image_metrics" else SB.ssim_cases())]
    assert sorted(want[entry]) == sorted(cases) and len(set(cases)) == len(cases)       # the fixture holds this table, every case once
    per = SB.B * (2 if entry == "image_metrics" else 1)
    bad = [(n, want[entry][n], got[entry][n]) for n in cases if got[entry][n] != want[entry][n]]
    print(f"\n{entry}: {len(cases)} cases x {per} values, {len(bad)} differ")
    assert all(len(want[entry][n]) == per for n in cases)
    assert not bad, bad[:4]
