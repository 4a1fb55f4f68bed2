"""The colour view of the on-device games (GridBreakout, GridBoxing): what a simulator's
current game looks like to a person, with the policy's output under it.  This module states the
image ONCE, over the games' own `render_numpy` and `PALETTE`; it restates no rule of either game
and is the oracle of the HIP kernel (csrc/ba3c_envview.h: env_view_kernel, behind
ba3c_breakout_view / ba3c_boxing_view, reached through `BreakoutVec.view` / `BoxingVec.view`).

The canvas is 84 px wide and Hc = 84 px high, or Hc = 84 + HUD_H with a HUD.  Canvas rows 0..83
are `palette[render_numpy(row)]`.  The HUD strip is drawn from 20 bytes per image (integers
only, so that the GPU can be held to it exactly):

    hud[0..17]   the bar heights of actions 0..17, clamped to BAR_MAX = 16
    hud[18]      the chosen action; 255 (or anything >= 18): none
    hud[19]      the length of the value bar, clamped to 84

and, with yy the row inside the strip and every pixel not named below HUD_BG:

    yy = 0       the separator: HUD_SEP for every x
    yy = 1, 2    the value bar: HUD_VALUE where x < hud[19]
    yy = 3       blank
    yy = 4..19   the action bars: action a covers x in [6 + 4a, 6 + 4a + 3) and is lit where
                 19 - yy < hud[a], HUD_HI if a == hud[18] else HUD_LO

Scale S in [1, 8]: out[y*S + dy, x*S + dx] = canvas[y, x].  `sel` picks the simulators, in any
order and with repeats; an entry outside [0, E) yields an all-zero image (HUD included).
"""
import numpy as np

W = 84
HUD_H = 20
HUD_BYTES = 20
MAX_SCALE = 8
ACTIONS = 18                 # bars in the strip: ALE's full action set
BAR_X0, BAR_PITCH, BAR_W, BAR_MAX, BAR_Y0 = 6, 4, 3, 16, 4
NO_ACTION = 255
HUD_BG = (0, 0, 0)
HUD_SEP = (96, 96, 96)
HUD_VALUE = (80, 200, 255)
HUD_LO = (60, 140, 200)
HUD_HI = (80, 255, 80)


def check_scale(scale):
    if not isinstance(scale, (int, np.integer)) or not 1 <= scale <= MAX_SCALE:
        raise ValueError("scale must be an integer in [1, %d], got %r" % (MAX_SCALE, scale))
    return int(scale)


def _game_of(palette):
    """The game module whose PALETTE this is (the view is built on ITS render_numpy)."""
    from . import boxing, breakout
    for mod in (breakout, boxing):
        if np.array_equal(palette, mod.PALETTE):
            return mod
    raise ValueError("palette is neither game's PALETTE: pass game=<module>")


def hud_strip_numpy(hud):
    """[n, HUD_H, 84, 3] uint8: the strip of each row of `hud` (uint8 [n, 20])."""
    hud = np.asarray(hud)
    if hud.dtype != np.uint8 or hud.ndim != 2 or hud.shape[1] != HUD_BYTES:
        raise ValueError("hud must be uint8 [n, %d]" % HUD_BYTES)
    n = hud.shape[0]
    strip = np.zeros((n, HUD_H, W, 3), np.uint8)
    strip[...] = HUD_BG
    strip[:, 0] = HUD_SEP
    x = np.arange(W)
    value = x[None, :] < np.minimum(hud[:, 19].astype(np.int64), W)[:, None]          # [n,W]
    strip[:, 1:3][np.broadcast_to(value[:, None, :], (n, 2, W))] = HUD_VALUE
    yy = np.arange(BAR_Y0, HUD_H)
    for a in range(ACTIONS):
        height = np.minimum(hud[:, a].astype(np.int64), BAR_MAX)
        lit = (HUD_H - 1 - yy)[None, :] < height[:, None]                             # [n,16]
        colour = np.where((hud[:, 18] == a)[:, None], HUD_HI, HUD_LO).astype(np.uint8)  # [n,3]
        x0 = BAR_X0 + BAR_PITCH * a
        bar = strip[:, BAR_Y0:, x0:x0 + BAR_W]                                        # a view
        bar[...] = np.where(lit[:, :, None, None], colour[:, None, None, :], bar)
    return strip


def view_numpy(game_rows, palette, scale=1, hud=None, sel=None, game=None):
    """uint8 [n, Hc*scale, 84*scale, 3]: the colour view of `game_rows` ([E,16] int32) under
    `palette` (uint8 [256,3]; the game is the one whose PALETTE it is, unless `game` names the
    module).  hud: uint8 [n, 20] or None; sel: int32 [n] or None (0..E-1)."""
    S = check_scale(scale)
    palette = np.asarray(palette)
    if palette.dtype != np.uint8 or palette.shape != (256, 3):
        raise ValueError("palette must be uint8 [256, 3]")
    mod = game if game is not None else _game_of(palette)
    rows = np.asarray(game_rows)
    E = rows.shape[0]
    sel = np.arange(E, dtype=np.int64) if sel is None else np.asarray(sel).astype(np.int64).reshape(-1)
    n = sel.shape[0]
    ok = (sel >= 0) & (sel < E)
    canvas = palette[mod.render_numpy(rows[np.where(ok, sel, 0)])]       # uint8 shades: in the table
    if hud is not None:
        strip = hud_strip_numpy(hud)
        if strip.shape[0] != n:
            raise ValueError("hud has %d rows for %d images" % (strip.shape[0], n))
        canvas = np.concatenate([canvas, strip], axis=1)
    canvas[~ok] = 0
    return np.repeat(np.repeat(canvas, S, axis=1), S, axis=2)


def hud_from_policy(probs, actions, value):
    """The HUD bytes (uint8 [n, 20]) of a policy's output: probs float [n, A] (A <= 18),
    actions int [n] or None, value float [n] or None (a bar of 42: v = 0).  A few torch ops on
    the inputs' device; torch's round on both, so CPU and device tensors give the same bytes."""
    import torch
    n, A = probs.shape
    if A > ACTIONS:
        raise ValueError("the HUD has %d bars, got %d actions" % (ACTIONS, A))
    hud = torch.zeros((n, HUD_BYTES), dtype=torch.uint8, device=probs.device)
    hud[:, :A] = torch.round(probs.to(torch.float32) * BAR_MAX).clamp(0, BAR_MAX).to(torch.uint8)
    if actions is None:
        hud[:, 18] = NO_ACTION
    else:
        a = actions.to(device=probs.device, dtype=torch.int64)
        hud[:, 18] = torch.where((a >= 0) & (a < ACTIONS), a, torch.full_like(a, NO_ACTION)).to(torch.uint8)
    v = torch.zeros(n, dtype=torch.float32, device=probs.device) if value is None else value.to(
        device=probs.device, dtype=torch.float32).reshape(n)
    hud[:, 19] = torch.round(42.0 + 42.0 * torch.tanh(v)).clamp(0, W).to(torch.uint8)
    return hud


def device_view(vec, fn, palette, scale=1, sel=None, hud=None, n_rows=None, rows=None):
    """`BreakoutVec.view` / `BoxingVec.view`: one launch of `fn` (the game's ba3c_*_view) over
    vec.game -> torch.uint8 [n, Hc*scale, 84*scale, 3] on the device.  The palette is uploaded
    by the first call and kept on `vec`; nothing else of `vec` is written.  n_rows: the rows of
    vec.game where that is not vec.E (BoxingDuelVec: two players per row); rows: a device tensor
    shaped like vec.game to draw in its place (BoxingDuelVec's mirrored rows)."""
    torch = vec._torch
    S = check_scale(scale)
    if vec._palette is None:
        vec._palette = torch.from_numpy(np.array(palette, np.uint8)).to(vec.device)
    n_rows = vec.E if n_rows is None else int(n_rows)
    n = n_rows
    if sel is not None:
        sel = torch.as_tensor(sel).to(device=vec.device, dtype=torch.int32).contiguous().reshape(-1)
        n = sel.shape[0]
    if hud is not None:
        hud = torch.as_tensor(hud)
        if hud.dtype != torch.uint8 or tuple(hud.shape) != (n, HUD_BYTES):
            raise ValueError("hud must be uint8 [%d, %d]" % (n, HUD_BYTES))
        hud = hud.to(vec.device).contiguous()
    if n < 1:
        raise ValueError("sel is empty")
    hc = W + (HUD_H if hud is not None else 0)
    out = torch.empty((n, hc * S, W * S, 3), dtype=torch.uint8, device=vec.device)
    ptr = vec._ptr
    vec._check(fn(vec._stream(), ptr(vec.game if rows is None else rows), n_rows, ptr(sel), n, ptr(vec._palette), ptr(hud), S,
                  ptr(out)))
    return out
