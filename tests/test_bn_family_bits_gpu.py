"""The BatchNorm / LeakyReLU / max-pool passes leave the bits of the build that preceded their rewrite around shared
helpers (tests/golden/bn_family_bits.json, cases in tests/bn_family_cases.py), and the backward pass takes the pool
widths it has kernels for and refuses the others before anything runs."""
import json

import pytest
import torch

from pitchextractor_amd import ops
from tests import bn_family_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def recorded(golden_dir):
    return json.loads((golden_dir / "bn_family_bits.json").read_text())


def test_every_case_is_recorded(recorded):
    assert sorted(recorded) == sorted(cases.CASES)


@pytest.mark.parametrize("name", sorted(cases.CASES))
def test_pass_leaves_the_recorded_bits(hip_device, recorded, name):
    got = {k: cases.digest(v) for k, v in cases.run_case(ops, name, hip_device).items()}
    assert got == recorded[name]


@pytest.mark.parametrize("dt", [torch.float32, torch.bfloat16], ids=["fp32", "bf16"])
def test_backward_refuses_other_pool_widths_on_the_host(hip_device, dt):
    """pool = 5: a ValueError before any launch, for both storage types; dx keeps what it held."""
    dev, C = hip_device, 64
    x = cases.bf16_values(1, 1, 3, 20, C).to(dt).to(dev)
    dy = cases.bf16_values(2, 1, 3, 4, C).to(dt).to(dev)
    st = ops.bn_train_stats(x, torch.ones(C, device=dev), torch.zeros(C, device=dev), None, None)
    dg, db = torch.full((C,), 3.0, device=dev), torch.full((C,), 3.0, device=dev)
    dx = torch.full_like(x, 5.0)
    word = torch.zeros(1, dtype=torch.int32, device=dev)
    with pytest.raises(ValueError):
        ops.bn_act_pool_bwd(x, dy, st, dg, db, pool=5, dx=dx, amax_out=word)
    torch.cuda.synchronize()
    assert torch.equal(dx, torch.full_like(x, 5.0)) and word.item() == 0
    assert torch.equal(dg, torch.full_like(dg, 3.0)) and torch.equal(db, torch.full_like(db, 3.0))
