"""Nine of the stored launch traces (tests/stack_trace.py) on the device: real inputs, a valid random idx, the launches
seen by a `_lib._hooks` hook -- the same trace as the stored one, and finite outputs."""
import pytest
import torch

import stack_trace as ST

pytestmark = pytest.mark.gpu
GOLDEN = ST.load_golden()


@pytest.mark.parametrize("name", ST.GPU_CASES)
def test_device_trace_equals_the_stored_one(name):
    torch.manual_seed(len(name))
    trace, _, outs = ST.run_case(name, dev="cuda:0", recorder=ST.hooked)
    torch.cuda.synchronize()
    assert trace == ST.hook_view(GOLDEN[name])
    assert all(torch.isfinite(o).all().item() for o in outs)
