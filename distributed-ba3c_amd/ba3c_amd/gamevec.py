"""GameVec: what the on-device games' vectors share (BreakoutVec, BoxingVec, BoxingDuelVec,
BoxingDuelDecisionVec): G rows of `game` in HBM for E = PLAYERS * G players with SyntheticAtari's
interface (`E`, `A`, `frames()`, `step(actions) -> frames, reward, over`); every step is one HIP
launch (STEP).  `step_into(actions, hist)` also pushes the new frames into a
FrameHistory(hist_len=4, channels=1) in that same launch.  `last_ep_score` / `last_over` expose
the episodes the last step finished.  With a setting in `skip` (lo, hi, q16) every step is one
DECISION (ba3c_amd.frameskip), still one launch (DECIDE), with the aux rows in `aux`; `limit`
counts game steps either way.  Every per-player tensor (actions in; reward, over, ep_score,
frame, state out) has E rows, player p of row e at p * G + e.

A game's vector is a subclass that declares
    A, PALETTE                   the number of actions and the colours of ba3c_amd.view
    STEP, DECIDE, RENDER, VIEW   the names of its entry points (include/ba3c.h)
    initial_game(n, seed)        its module's fresh rows [n,16] int32
    initial_aux(n, seed)         its module's fresh aux rows (default: ba3c_amd.frameskip's)
    PLAYERS, COUNT               players per row and the rows' name, where not 1 and "n_envs"
"""
import ctypes

from . import frameskip

H = W = 84
DEFAULT_LIMIT = 40000                # LimitLengthPlayer(40000), train.py:127


class GameVec(object):
    PLAYERS = 1
    COUNT = "n_envs"
    initial_aux = staticmethod(frameskip.initial_aux)
    # (lo, hi, q16) of ba3c_amd.frameskip, or None: the plain one-step launch and no aux rows;
    # start: what DECIDE takes after them (the duel's drawn start), if anything
    skip = start = aux = None

    def __init__(self, n_envs, seed=0, limit=DEFAULT_LIMIT, device="cuda", frame_skip=1, sticky=0.0):
        self._counts(n_envs, limit)
        self.skip = frameskip.setting(frame_skip, sticky)
        self._alloc(seed, device)

    def _counts(self, n_rows, limit):
        self.G = int(n_rows)
        self.E = self.PLAYERS * self.G
        self.limit = int(limit)
        if self.G < 1 or self.limit < 1:
            raise ValueError("%s and limit must be >= 1" % self.COUNT)

    def _alloc(self, seed, device):
        import torch

        from . import _lib
        self.lib = _lib.load()
        self._check = _lib.check
        self._torch = torch
        self.device = dev = torch.device(device)
        self.game = torch.from_numpy(self.initial_game(self.G, seed)).to(dev)
        if self.skip is not None:
            self.aux = torch.from_numpy(self.initial_aux(self.G, seed)).to(dev)
        self.reward = torch.zeros(self.E, dtype=torch.float64, device=dev)
        self.over = torch.zeros(self.E, dtype=torch.uint8, device=dev)
        self.ep_score = torch.zeros(self.E, dtype=torch.int32, device=dev)
        self.frame = torch.zeros((self.E, H, W, 1), dtype=torch.uint8, device=dev)
        self._palette = None               # PALETTE on the device, uploaded by the first view()

    def _ptr(self, t):
        return ctypes.c_void_p(t.data_ptr()) if t is not None else None

    def _stream(self):
        return ctypes.c_void_p(self._torch.cuda.current_stream().cuda_stream)

    def _actions(self, actions):
        a = actions.to(device=self.device, dtype=self._torch.int64).contiguous()
        assert a.shape == (self.E,)
        return a

    def _render(self, frame, state):
        self._check(getattr(self.lib, self.RENDER)(self._stream(), self._ptr(self.game), self.G,
                                                   self._ptr(frame), self._ptr(state)))

    def frames(self):
        """[E,84,84,1] uint8 frames of the current state, each player's own (a new tensor)."""
        out = self._torch.empty_like(self.frame)
        self._render(out, None)
        return out

    def reset_history(self, hist):
        """Start `hist` (FrameHistory 4x1 over the E players) from the current frames: zeros +
        frame."""
        self._check_hist(hist)
        self._render(None, hist.state)
        return hist.state

    def _check_hist(self, hist):
        if (hist.H, hist.c, hist.E) != (4, 1, self.E) or not hist.state.is_contiguous():
            raise ValueError("the fused push needs a FrameHistory(n_envs=%d, hist_len=4, channels=1)"
                             % self.E)

    def _step(self, actions, frame, state):
        ptr = self._ptr
        a = self._actions(actions)
        outs = (ptr(self.reward), ptr(self.over), ptr(self.ep_score), ptr(frame), ptr(state))
        if self.skip is None:
            self._check(getattr(self.lib, self.STEP)(self._stream(), ptr(self.game), ptr(a), self.G,
                                                     self.limit, *outs))
        else:
            setting = tuple(self.skip) + tuple(self.start or ())
            self._check(getattr(self.lib, self.DECIDE)(self._stream(), ptr(self.game), ptr(self.aux), ptr(a),
                                                       self.G, self.limit, *(setting + outs)))
        return self.reward, self.last_over

    def step(self, actions):
        """-> (frames [E,84,84,1] uint8, reward float64 [E], over bool [E]); the tensors are
        this object's buffers, overwritten by the next step."""
        reward, over = self._step(actions, self.frame, None)
        return self.frame, reward, over

    def step_into(self, actions, hist):
        """Step and push every player's new frame into `hist.state` in the same launch.
        -> (reward float64 [E], over bool [E])."""
        self._check_hist(hist)
        return self._step(actions, None, hist.state)

    def view(self, scale=1, sel=None, hud=None, rows=None):
        """The colour view of the current rows (ba3c_amd.view.view_numpy is its statement):
        torch.uint8 [n, Hc*scale, 84*scale, 3] on the device, one launch (VIEW); sel: row
        indices (None: all G), hud: uint8 [n, 20] or None; rows: a tensor to draw in place of
        `game`.  Reads `game` only."""
        from .view import device_view
        return device_view(self, getattr(self.lib, self.VIEW), self.PALETTE, scale, sel, hud, n_rows=self.G,
                           rows=rows)

    @property
    def last_over(self):
        return self.over.view(self._torch.bool)

    @property
    def last_ep_score(self):
        """(ep_score int32 [E], over bool [E]) of the last step: ep_score[p] is player p's score
        of the finished episode where over[p], stale elsewhere."""
        return self.ep_score, self.last_over
