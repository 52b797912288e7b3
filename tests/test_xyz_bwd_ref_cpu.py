"""tests/xyz_bwd_ref.py, the float64 restatement tests/test_xyz_bwd_tiles_gpu.py holds the kernels to, checked without a GPU:
(a) against float64 autograd of the graph it restates, (b) that the shared inputs make the ReLU decision exact in fp32 -- the
condition that keeps a mask flip from hiding in a tolerance -- and (c) that a wrong restatement is told apart."""
import pytest
import torch

import xyz_bwd_ref as XR

K = XR.K
ROW_COUNTS = (65536, 65537, 65599, 65601)          # the row counts of the GPU file


def _autograd(d):
    """off -> y1 -> BN-affine + ReLU -> . W (+ bias) -> contracted with the fixed cotangent dY; -> the restatement's dict"""
    f = {k: v.double() for k, v in d.items()}
    off, xw = f["off4"][:, :3], f["xyzw"]
    asc, ash, W = f["asc"].clone().requires_grad_(), f["ash"].clone().requires_grad_(), f["W"].clone().requires_grad_()
    bias = torch.zeros(W.shape[1], dtype=torch.float64, requires_grad=True)
    y1 = off @ xw[:3] + xw[3]
    z = y1 * asc + ash
    z.retain_grad()
    out = torch.relu(z) @ W + bias
    cot = f["p"] * f["G"] + f["q"] * f["Y"] + f["t"]
    (out * cot).sum().backward()
    # d/d a_shift = sum Gp, d/d a_scale = sum Gp y1; the offsets' sums from the gradient at z itself
    return {"dW": W.grad, "db": bias.grad, "gp": ash.grad, "gpy": asc.grad, "off": off.t() @ z.grad}


def _wrong(d, kind):
    f = {k: v.double() for k, v in d.items()}
    off, xw = f["off4"][:, :3], f["xyzw"]
    y1 = off @ xw[:3] + xw[3]
    z = y1 * f["asc"] + f["ash"]
    dY = f["p"] * f["G"] + f["q"] * f["Y"] + (0.0 if kind == "no_t" else f["t"])
    mask = ((y1 if kind == "mask_on_y1" else z) > 0).double()
    Wt = f["W"] if kind == "w_for_wt" else f["W"].t()
    Gp = (dY @ Wt) * mask
    return {"dW": z.clamp_min(0.0).t() @ dY, "db": dY.sum(0), "gp": Gp.sum(0), "gpy": (Gp * y1).sum(0), "off": off.t() @ Gp}


def _worst(a, b):
    return max(((a[k] - b[k]).abs().max() / b[k].abs().max().clamp_min(1e-300)).item() for k in b)


@pytest.mark.parametrize("kind", XR.KINDS)
def test_restatement_equals_autograd(kind):
    d = XR.make_inputs(1031, 64, seed=3, kind=kind)
    got, want = XR.reference(d), _autograd(d)
    for k in want:
        scale = want[k].abs().max().item()
        err = (got[k] - want[k]).abs().max().item()
        assert err <= 1e-10 * max(scale, 1.0), "%s: %.3e of %.3e" % (k, err, scale)


def test_restatement_equals_autograd_at_128_columns():
    d = XR.make_inputs(517, 128, seed=4)
    got, want = XR.reference(d), _autograd(d)
    for k in want:
        assert (got[k] - want[k]).abs().max().item() <= 1e-10 * max(want[k].abs().max().item(), 1.0), k


@pytest.mark.parametrize("M", ROW_COUNTS)
def test_relu_decision_is_exact_in_fp32_random_sets(M):
    d = XR.make_inputs(M, 64, seed=M % 1000)
    z32, z64 = XR.z_fp32(d), XR.z_fp64(d)
    assert z32.dtype == torch.float32 and torch.equal(z32.double(), z64)
    assert (z64 > 0).any() and (z64 < 0).any() and (z64 == 0).any()


@pytest.mark.parametrize("kind", XR.KINDS[1:])
def test_relu_decision_is_exact_in_fp32_hand_made_sets(kind):
    d = XR.make_inputs(65536, 64, seed=11, kind=kind)
    z32, z64 = XR.z_fp32(d), XR.z_fp64(d)
    assert torch.equal(z32.double(), z64)
    if kind == "masks_off":
        assert (z64 < 0).all()
    elif kind == "masks_on":
        assert (z64 > 0).all()
    else:
        assert (z64 > 0).any() and (z64 < 0).any() and (z64 == 0).any()


def test_relu_decision_is_exact_at_both_widths():
    for N in (64, 128):
        d = XR.make_inputs(65536, N, seed=21)
        assert torch.equal(XR.z_fp32(d).double(), XR.z_fp64(d))


@pytest.mark.parametrize("kind", ("mask_on_y1", "no_t", "w_for_wt"))
def test_wrong_restatement_is_rejected(kind):
    d = XR.make_inputs(1031, 64, seed=5)
    want = _autograd(d)
    assert _worst(XR.reference(d), want) <= 1e-10
    assert _worst(_wrong(d, kind), want) > 1e-3, kind
