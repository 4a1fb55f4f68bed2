// ba3c_envview.h — the colour viewer of the on-device games: draw the CURRENT game of selected
// simulators as an RGB image, at an integer scale, with an optional HUD strip (the policy's
// output) under it.  ba3c_amd/view.py states the image once (view_numpy: the oracle of this
// kernel, over the games' own render_numpy); this file restates the palette lookup, the HUD
// strip and the scaling, and takes the game's pixels from the same `Rules` sim_kernel uses
// (ba3c_envkernel.h).  It lives in a header of its own so that the six step kernels compile
// exactly as they did without it.
//
// Image i shows simulator sel[i] (sel null: i); an index outside [0, n_envs) gives an all-zero
// image.  The canvas is 84 px wide and 84 (+ VIEW_HUD_H with a HUD) high; canvas pixel (y, x)
// fills the scale x scale block at (y*scale, x*scale) of the [Hc*scale][84*scale][3] output.
//
// One 256-thread workgroup per image.  A thread takes 4 canvas pixels of one canvas row (the
// group env_render_push takes), so a game pixel is computed once whatever the scale, and writes
// their 12*scale bytes of each of the `scale` output rows as dwords: an output row is
// 252*scale bytes, a multiple of 4 for every scale but of 16 only for scale 4 and 8.
// The kernel reads the game row, sel, hud and the palette and writes nothing but `out`.
#pragma once
#include "ba3c_envkernel.h"

namespace ba3c {

constexpr int VIEW_HUD_H = 20, VIEW_HUD_BYTES = 20, VIEW_MAX_SCALE = 8, VIEW_ACTIONS = 18;
constexpr int VIEW_BAR_X0 = 6, VIEW_BAR_PITCH = 4, VIEW_BAR_W = 3, VIEW_BAR_MAX = 16, VIEW_BAR_Y0 = 4;
// colours as r | g << 8 | b << 16 (view.py: HUD_SEP, HUD_VALUE, HUD_LO, HUD_HI)
constexpr uint32_t VIEW_SEP = 0x00606060u, VIEW_VALUE = 0x00FFC850u, VIEW_LO = 0x00C88C3Cu,
                   VIEW_HI = 0x0050FF50u;

struct ViewArgs {
  const int32_t* game;      // [E][16]
  int32_t n_envs;
  const int32_t* sel;       // [n] or null
  const uint8_t* palette;   // [256][3]
  const uint8_t* hud;       // [n][20] or null
  int32_t scale;            // in [1, 8] (checked by the host)
  uint8_t* out;             // [n][Hc*scale][84*scale][3]
};

// view.py: the HUD strip, for pixel (yy, x) of the strip; h = the image's 20 HUD bytes.  A bar
// height indexes nothing, and h is indexed by an action below VIEW_ACTIONS only.
__device__ __forceinline__ uint32_t view_hud_pixel(const uint8_t* h, int yy, int x) {
  if (yy == 0) return VIEW_SEP;
  if (yy < 3) return x < min((int)h[19], ENV_W) ? VIEW_VALUE : 0u;
  const int t = x - VIEW_BAR_X0;
  if (yy < VIEW_BAR_Y0 || t < 0) return 0u;
  const int act = t / VIEW_BAR_PITCH;
  if (act >= VIEW_ACTIONS || t - act * VIEW_BAR_PITCH >= VIEW_BAR_W) return 0u;
  if (VIEW_HUD_H - 1 - yy >= min((int)h[act], VIEW_BAR_MAX)) return 0u;
  return act == (int)h[18] ? VIEW_HI : VIEW_LO;
}

// c0..c3 by selects: a dynamically indexed private array would be placed in scratch
__device__ __forceinline__ uint32_t view_pick(int i, uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3) {
  return i == 0 ? c0 : i == 1 ? c1 : i == 2 ? c2 : c3;
}

template <class Rules>
__global__ void __launch_bounds__(256) env_view_kernel(const ViewArgs a) {
  __shared__ uint32_t pal[256];
  const int i = blockIdx.x;
  const int tid = threadIdx.x;
  const int32_t s = a.sel ? a.sel[i] : i;
  const bool valid = (uint32_t)s < (uint32_t)a.n_envs;
  const int e = valid ? s : 0;          // out of range: row 0 is read and every colour is 0
  const int4* row = reinterpret_cast<const int4*>(a.game + (size_t)e * 16);
  const int4 r0 = row[0], r1 = row[1], r2 = row[2], r3 = row[3];
  typename Rules::Game g;
  Rules::load(g, r0, r1, r2, r3);
  const uint8_t* p = a.palette + 3 * tid;
  pal[tid] = valid ? (uint32_t)p[0] | ((uint32_t)p[1] << 8) | ((uint32_t)p[2] << 16) : 0u;
  __syncthreads();
  const int S = a.scale;
  const int hc = ENV_W + (a.hud ? VIEW_HUD_H : 0);
  const uint8_t* h = a.hud ? a.hud + (size_t)i * VIEW_HUD_BYTES : nullptr;
  const int row_words = (ENV_W * 3 / 4) * S;                    // 63 * S dwords per output row
  uint32_t* out = reinterpret_cast<uint32_t*>(a.out) + (size_t)i * hc * S * row_words;
  for (int q = tid; q < hc * (ENV_W / 4); q += 256) {
    const int y = q / (ENV_W / 4), x0 = 4 * (q - y * (ENV_W / 4));
    uint32_t c0, c1, c2, c3;
    if (y < ENV_W) {
      const typename Rules::Row rw = Rules::row(g, y);
      c0 = pal[Rules::pixel(g, y, x0, rw) & 255u];
      c1 = pal[Rules::pixel(g, y, x0 + 1, rw) & 255u];
      c2 = pal[Rules::pixel(g, y, x0 + 2, rw) & 255u];
      c3 = pal[Rules::pixel(g, y, x0 + 3, rw) & 255u];
    } else {
      const int yy = y - ENV_W;
      c0 = valid ? view_hud_pixel(h, yy, x0) : 0u;
      c1 = valid ? view_hud_pixel(h, yy, x0 + 1) : 0u;
      c2 = valid ? view_hud_pixel(h, yy, x0 + 2) : 0u;
      c3 = valid ? view_hud_pixel(h, yy, x0 + 3) : 0u;
    }
    // the 4 canvas pixels are 4*S output pixels = S groups of 4 px = 3 dwords each
    uint32_t* dst = out + (size_t)y * S * row_words + (x0 / 4) * 3 * S;
    int src = 0, rep = 0;               // output pixel 4m+k shows canvas pixel src = (4m+k) / S
    for (int m = 0; m < S; ++m) {
      uint32_t px[4];
#pragma unroll
      for (int k = 0; k < 4; ++k) {
        px[k] = view_pick(src, c0, c1, c2, c3);
        if (++rep == S) { rep = 0; ++src; }
      }
      const uint32_t w0 = px[0] | (px[1] << 24);
      const uint32_t w1 = (px[1] >> 8) | (px[2] << 16);
      const uint32_t w2 = (px[2] >> 16) | (px[3] << 8);
      for (int dy = 0; dy < S; ++dy) {
        uint32_t* d = dst + dy * row_words + 3 * m;
        d[0] = w0;
        d[1] = w1;
        d[2] = w2;
      }
    }
  }
}

}  // namespace ba3c
