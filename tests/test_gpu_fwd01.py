"""conv0's and conv1's forward as one persistent launch (fwd01_kernel, BA3C_FWD01=1, the default)
against the two launches it replaces (BA3C_FWD01=0), bit for bit.

The fused launch runs wherever conv1's forward is the ring walk: B >= 2 CUs and (B % (2 CUs) == 0
or B >= 16 CUs).  Inside it a workgroup's conv1 reads the p0 rows and the per-image maximum its
own conv0 wrote a moment earlier in the same launch; a stale maximum gives a wrong operand scale
and still finite numbers.  With tests/mixed_frames.py neighbouring images sit in different binades
and some are black, so a maximum read from a line fetched for the neighbour changes bits.

* B = 2 CUs (one image per workgroup) and B = 4 CUs (two: the hand-back from conv1 to conv0 and
  the second maximum), training pass and predictor: every forward map, the flat gradients and the
  eight scalars torch.equal between the two settings;
* B = 2 CUs + 1 does not take the fused launch: kernel_merged("conv0_fwd") is empty for it;
* ba3c_create rejects any BA3C_FWD01 value but 0 and 1.

One handle geometry (F=128, S=4, A=4); no CPU oracle.
"""
import numpy as np
import pytest
import torch

from oracle import ba3c_oracle as O
from mixed_frames import mixed_frames

pytestmark = pytest.mark.gpu

F, S, A = 128, 4, 4
MAPS = ("p0", "c0", "p1", "c1", "p2", "a3")
_ENG = {}


def _cus():
    return torch.cuda.get_device_properties(torch.cuda.current_device()).multi_processor_count


def _engines(monkeypatch):
    """The handles with BA3C_FWD01 = 1 and 0 (ba3c_create reads the switch), same parameters."""
    if not _ENG:
        from ba3c_amd.engine import Ba3cEngine
        params = O.init_params(F, S, A, seed=11, dtype=np.float32)
        for val in ("1", "0"):
            monkeypatch.setenv("BA3C_FWD01", val)
            eng = Ba3cEngine(num_actions=A, fc_neurons=F, fc_splits=S, max_batch=4 * _cus())
            eng.load_params(params)
            _ENG[val] = eng
        monkeypatch.delenv("BA3C_FWD01")
    return _ENG["1"], _ENG["0"]


def _frames(kind, B):
    if kind == "mixed":
        return mixed_frames(B, 23)[0]
    return np.random.RandomState(B).randint(0, 256, size=(B, 84, 84, 4)).astype(np.uint8)


def _batches():
    n = _cus()
    return {"one_image": 2 * n, "two_images": 4 * n, "unfused": 2 * n + 1}


def _run(eng, state, action, R, B):
    sc = eng.train_grads(state, action, R, entropy_beta=0.01)
    out = {n: eng.workspace_tensor(n, B).clone() for n in MAPS}
    out["grads"] = eng.grads.clone()
    out["scalars"] = sc.clone()
    merged = eng.kernel_merged("conv0_fwd")
    probs, _, value = eng.forward(state)
    out["probs"], out["value"] = probs.clone(), value.clone()
    return out, merged


@pytest.mark.parametrize("val", ["2", "on", ""])
def test_switch_rejects_other_values(monkeypatch, val):
    from ba3c_amd import Ba3cLibraryError
    from ba3c_amd.engine import Ba3cEngine
    monkeypatch.setenv("BA3C_FWD01", val)
    with pytest.raises(Ba3cLibraryError, match="BA3C_FWD01"):
        Ba3cEngine(num_actions=A, fc_neurons=F, fc_splits=S, max_batch=8)


@pytest.mark.parametrize("kind", ["random", "mixed"])
@pytest.mark.parametrize("size", ["one_image", "two_images", "unfused"])
def test_fused_forward_is_bit_identical_to_two_launches(monkeypatch, size, kind):
    on, off = _engines(monkeypatch)
    B = _batches()[size]
    rs = np.random.RandomState(B + 1)
    state = torch.from_numpy(_frames(kind, B)).cuda()
    action = torch.from_numpy(rs.randint(0, A, size=B).astype(np.int64)).cuda()
    R = torch.from_numpy(rs.normal(size=B).astype(np.float32)).cuda()
    got, m_on = _run(on, state, action, R, B)
    ref, m_off = _run(off, state, action, R, B)
    assert m_off == []
    assert m_on == ([] if size == "unfused" else ["conv1_fwd"])
    for k in ref:
        assert torch.equal(got[k], ref[k]), (size, kind, k)
    assert on.device_errors() == 0 and off.device_errors() == 0
