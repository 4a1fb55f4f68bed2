// ba3c_gridpong.h — GridPong: a small integer-only Pong for a vector of simulators: ALE Pong's 6
// actions, a tracking opponent that lapses, +1 / -1 per point, first to 21.  The rules are stated
// once in ba3c_amd/gridpong.py (constants, step_numpy, render_numpy: the oracle of this kernel);
// this file restates them.
//
// game[e] = [py, oy, bx, by, vx, vy, mine, theirs, t, rng, hits, serve, 0, 0, 0, 0],
// 16 int32 = 64 bytes; py / oy: the agent's (right) / the opponent's (left) paddle top in pixels,
// (bx, by) / (vx, vy): the ball in eighths of a pixel (per step).
//
// The launch is sim_kernel<SoloSim<PongRules>, .> (ba3c_envkernel.h: one 256-thread workgroup per
// simulator, the skeleton the other games share); this file holds the game's step and pixel rules.
//
// Step: wave-uniform, so it lives in scalar registers for the k steps of a decision.  Both
// branches of the rules (a row that waits for its serve, a row in play) are computed and the row
// takes one of them by selects; reflections, the two paddles and the two ways to score are
// selects too, so a decision's loop body is one basic block.
// Render: per frame row the scene is three unsigned spans [lo, lo + w) (the agent's, the
// opponent's, the ball's) and a flag word (wall row, net dash row).  The score bars lie in rows
// no paddle reaches (a paddle's rows are 12..81), and each has its owner's shade, so a bar IS its
// owner's span in those rows.  A pixel is three range compares, one more for the net, and selects.
#pragma once
#include "ba3c_envkernel.h"

namespace ba3c {

constexpr int PG_SUB = 3;                                   // eighths of a pixel
constexpr int PG_PADDLE_W = 2, PG_PADDLE_H = 10, PG_PADDLE_STEP = 2, PG_OPP_STEP = 1;
constexpr int PG_AGENT_X = 76, PG_OPP_X = 6, PG_Y_MIN = 12, PG_Y_MAX = 72, PG_PY0 = 42;
constexpr int PG_EDGE = 2 << PG_SUB;                        // the ball's side
constexpr int PG_BY_MIN = 12 << PG_SUB, PG_BY_MAX = 80 << PG_SUB;
constexpr int PG_AGENT_FACE = PG_AGENT_X << PG_SUB, PG_OPP_FACE = (PG_OPP_X + PG_PADDLE_W) << PG_SUB;
constexpr int PG_AGENT_PAST = (PG_AGENT_X + PG_PADDLE_W) << PG_SUB, PG_OPP_PAST = (PG_OPP_X << PG_SUB) - PG_EDGE;
constexpr int PG_BX0 = 41 << PG_SUB, PG_BY0 = 46 << PG_SUB, PG_CENTRE_ROW = 47;
constexpr int PG_V0 = 10, PG_V_STEP = 2, PG_V_CAP = 14, PG_HITS_SHIFT = 2;
// |vy| after a hit at d = 0..10 (ball row - paddle top + 1), four bits each (gridpong.py: VY_MAGS)
constexpr uint64_t PG_VY_TABLE = 0xC964212469Cull;
constexpr uint32_t PG_LAPSE_OF_8 = 2;
constexpr int PG_SERVE_DELAY = 16, PG_SERVE_TOP = 33, PG_SERVE_BOTTOM = 59, PG_WIN = 21;
// bit a of a mask: action a has that component (gridpong.py: UP_SET, DOWN_SET, FIRE_SET)
constexpr uint32_t PG_UP = 0x14u, PG_DOWN = 0x28u, PG_FIRE = 0x32u;
constexpr uint32_t PG_ROW_WALL = 1u, PG_ROW_NET = 2u;       // Row::flags
constexpr int PG_A_BAR_Y = 2, PG_O_BAR_Y = 5, PG_BAR_UNIT = 4, PG_WALL_TOP = 10, PG_WALL_BOTTOM = 82;
constexpr int PG_NET_X = 41, PG_NET_W = 2;

struct PongGame {
  int32_t py, oy, bx, by, vx, vy, mine, theirs, t;
  uint32_t rng;
  int32_t hits, serve;
};

__device__ __forceinline__ int32_t pg_clamp(int32_t v, int32_t lo, int32_t hi) { return min(max(v, lo), hi); }

// One step of the rules (gridpong.py: step_numpy).  Returns the reward; *over_out / *ep_out as the
// entry point documents them.  `a` is range-checked and shifts the masks, never an index.
__device__ __forceinline__ int32_t pg_step(PongGame& g, int64_t a, int32_t limit, bool* over_out,
                                           int32_t* ep_out) {
  const uint32_t sh = (uint64_t)a < 6u ? (uint32_t)a : 0u;         // NOOP has no bit in any mask
  const int32_t dy = (int32_t)((PG_DOWN >> sh) & 1u) - (int32_t)((PG_UP >> sh) & 1u);
  const bool fire = (PG_FIRE >> sh) & 1u;
  g.rng = env_lcg(g.rng);
  const uint32_t r = g.rng >> 16;
  g.py = pg_clamp(g.py + PG_PADDLE_STEP * dy, PG_Y_MIN, PG_Y_MAX);
  const bool waiting = g.serve > 0;
  const int32_t target = waiting ? PG_CENTRE_ROW : (g.by >> PG_SUB) + 1;
  const int32_t ody = (r & 7u) < PG_LAPSE_OF_8 ? 0 : pg_clamp(target - (g.oy + PG_PADDLE_H / 2), -PG_OPP_STEP, PG_OPP_STEP);
  g.oy = pg_clamp(g.oy + ody, PG_Y_MIN, PG_Y_MAX);

  // a row that waits: count down; FIRE or the end of the count serves
  const int32_t w_serve = g.serve - 1;
  const bool now = fire || w_serve == 0;
  const int32_t k = (int32_t)((r >> 3) & 7u), m = 1 + (int32_t)((r >> 6) & 1u);
  const bool top = (r >> 7) & 1u;
  const int32_t s_by = (top ? PG_SERVE_TOP + k : PG_SERVE_BOTTOM - k) << PG_SUB, s_vy = top ? -m : m;

  // a row in play: move, the walls, the paddles' faces, the points
  int32_t nx = g.bx + g.vx, ny = g.by + g.vy;
  const bool lo_wall = ny < PG_BY_MIN, hi_wall = ny > PG_BY_MAX;
  ny = lo_wall ? 2 * PG_BY_MIN - ny : (hi_wall ? 2 * PG_BY_MAX - ny : ny);
  const int32_t wvy = (lo_wall || hi_wall) ? -g.vy : g.vy;
  const int32_t b = ny >> PG_SUB, da = b - g.py + 1, dob = b - g.oy + 1;
  const bool hit_a = g.vx > 0 && g.bx + PG_EDGE <= PG_AGENT_FACE && nx + PG_EDGE > PG_AGENT_FACE &&
                     (uint32_t)da <= (uint32_t)PG_PADDLE_H;
  const bool hit_o = g.vx < 0 && g.bx >= PG_OPP_FACE && nx < PG_OPP_FACE && (uint32_t)dob <= (uint32_t)PG_PADDLE_H;
  const bool hit = hit_a || hit_o;
  const int32_t d = hit_a ? da : (hit_o ? dob : 0);
  nx = hit_a ? 2 * (PG_AGENT_FACE - PG_EDGE) - nx : (hit_o ? 2 * PG_OPP_FACE - nx : nx);
  const int32_t hits_p = g.hits + (hit ? 1 : 0);
  const int32_t speed = min(PG_V0 + PG_V_STEP * (hits_p >> PG_HITS_SHIFT), PG_V_CAP);
  const int32_t mag = (int32_t)((PG_VY_TABLE >> (4 * d)) & 15u);   // a shifted constant, no memory
  const int32_t pvx = hit_a ? -speed : (hit_o ? speed : g.vx);
  const int32_t pvy = hit ? (d < PG_PADDLE_H / 2 ? -mag : mag) : wvy;
  const bool lost = nx >= PG_AGENT_PAST, won = nx <= PG_OPP_PAST, point = lost || won;
  const int32_t p_reward = lost ? -1 : (won ? 1 : 0);

  const int32_t reward = waiting ? 0 : p_reward;
  g.mine += (!waiting && won) ? 1 : 0;
  g.theirs += (!waiting && lost) ? 1 : 0;
  g.bx = waiting ? g.bx : (point ? PG_BX0 : nx);
  g.by = waiting ? (now ? s_by : g.by) : (point ? PG_BY0 : ny);
  g.vx = waiting ? g.vx : (lost ? PG_V0 : (won ? -PG_V0 : pvx));
  g.vy = waiting ? (now ? s_vy : g.vy) : (point ? 0 : pvy);
  g.hits = waiting ? g.hits : (point ? 0 : hits_p);
  g.serve = waiting ? (now ? 0 : w_serve) : (point ? PG_SERVE_DELAY : 0);
  g.t += 1;
  const bool over = g.mine >= PG_WIN || g.theirs >= PG_WIN || g.t >= limit;
  *over_out = over;
  *ep_out = g.mine - g.theirs;
  g.py = over ? PG_PY0 : g.py;
  g.oy = over ? PG_PY0 : g.oy;
  g.bx = over ? PG_BX0 : g.bx;
  g.by = over ? PG_BY0 : g.by;
  g.vx = over ? PG_V0 : g.vx;
  g.vy = over ? 0 : g.vy;
  g.mine = over ? 0 : g.mine;
  g.theirs = over ? 0 : g.theirs;
  g.t = over ? 0 : g.t;
  g.hits = over ? 0 : g.hits;
  g.serve = over ? PG_SERVE_DELAY : g.serve;
  return reward;
}

// The game as ba3c_envkernel.h's sim_kernel takes it.
struct PongRules {
  using Game = PongGame;
  // gridpong.py: render_numpy, for the pixels of one frame row: the agent's span (its paddle, or
  // its score bar in the bar's rows), the opponent's likewise, the ball's, and the flags.
  struct Row {
    int32_t a_lo, o_lo, b_lo;
    uint32_t a_w, o_w, b_w, flags;
  };
  static __device__ __forceinline__ void load(Game& g, int4 r0, int4 r1, int4 r2, int4) {
    g.py = r0.x; g.oy = r0.y; g.bx = r0.z; g.by = r0.w;
    g.vx = r1.x; g.vy = r1.y; g.mine = r1.z; g.theirs = r1.w;
    g.t = r2.x; g.rng = (uint32_t)r2.y; g.hits = r2.z; g.serve = r2.w;
  }
  static __device__ __forceinline__ void store(const Game& g, int4* out) {
    out[0] = make_int4(g.py, g.oy, g.bx, g.by);
    out[1] = make_int4(g.vx, g.vy, g.mine, g.theirs);
    out[2] = make_int4(g.t, (int32_t)g.rng, g.hits, g.serve);
    out[3] = make_int4(0, 0, 0, 0);
  }
  static __device__ __forceinline__ int32_t step(Game& g, int64_t a, int32_t limit, bool* over_out,
                                                 int32_t* ep_out) {
    return pg_step(g, a, limit, over_out, ep_out);
  }
  static __device__ __forceinline__ Row row(const Game& g, int y) {
    Row rw;
    const bool a_bar = (unsigned)(y - PG_A_BAR_Y) < 2u, o_bar = (unsigned)(y - PG_O_BAR_Y) < 2u;
    const uint32_t o_len = (uint32_t)(PG_BAR_UNIT * g.theirs);
    rw.a_lo = a_bar ? 0 : PG_AGENT_X;
    rw.a_w = a_bar ? (uint32_t)(PG_BAR_UNIT * g.mine)
                   : ((unsigned)(y - g.py) < (unsigned)PG_PADDLE_H ? (uint32_t)PG_PADDLE_W : 0u);
    rw.o_lo = o_bar ? ENV_W - (int32_t)o_len : PG_OPP_X;
    rw.o_w = o_bar ? o_len : ((unsigned)(y - g.oy) < (unsigned)PG_PADDLE_H ? (uint32_t)PG_PADDLE_W : 0u);
    rw.b_lo = g.bx >> PG_SUB;
    rw.b_w = (g.serve == 0 && (unsigned)(y - (g.by >> PG_SUB)) < 2u) ? 2u : 0u;
    const bool wall = (unsigned)(y - PG_WALL_TOP) < 2u || (unsigned)(y - PG_WALL_BOTTOM) < 2u;
    const bool net = (unsigned)(y - (PG_WALL_TOP + 2)) < (unsigned)(PG_WALL_BOTTOM - PG_WALL_TOP - 2) &&
                     ((y - (PG_WALL_TOP + 2)) & 4) == 0;
    rw.flags = (wall ? PG_ROW_WALL : 0u) | (net ? PG_ROW_NET : 0u);
    return rw;
  }
  static __device__ __forceinline__ uint32_t pixel(const Game&, int, int x, const Row& rw) {
    const bool bright = (unsigned)(x - rw.a_lo) < rw.a_w || (unsigned)(x - rw.b_lo) < rw.b_w;
    const bool opp = (unsigned)(x - rw.o_lo) < rw.o_w;
    const bool dim = (rw.flags & PG_ROW_WALL) || ((rw.flags & PG_ROW_NET) && (unsigned)(x - PG_NET_X) < (unsigned)PG_NET_W);
    return bright ? 255u : (opp ? 130u : (dim ? 60u : 0u));
  }
};

}  // namespace ba3c
