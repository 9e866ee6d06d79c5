// atari_screen.h -- GameState::computeFeature (atari/game_state.h:53-82,122-133) as ONE fixed float32 recipe, shared by
// the kernel (atari_screen.hip) and its host restatement (pybind/synth_atari.cc), which are therefore bit-identical:
//   v      = float((double)max(a, b) / 255.0)                         (a 256-entry table)
//   scale  = float(in - 1) / float(83); src = scale * dst             (per axis, align_corners = true)
//   i0     = min((int)src, in - 1), i1 = min(i0 + 1, in - 1), l1 = min(src - i0, 1), l0 = 1 - l1
//   y      = l0h * (l0w * x[i0h][i0w] + l1w * x[i0h][i1w]) + l1h * (l0w * x[i1h][i0w] + l1w * x[i1h][i1w])
//   g      = (0.21 R + 0.72 G) + 0.07 B;  out = (uint8_t)(g * 255)    (truncated)
// This is ATen's CPU upsample_bilinear2d formula; the reference's torch ops may order or contract differently per
// build, so against torch the result is within 1 per pixel, not bit-identical.  No FMA contraction anywhere.
// Indexed-colour screens (one palette index per pixel) enter the same recipe after the lookup: see indexed_max_pixel.
// Plain C++ apart from the HIP qualifiers: g++ compiles it for the host restatement.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define RELA_ATARI_HD __host__ __device__
#else
#define RELA_ATARI_HD
#endif

namespace rela_atari {

constexpr int kOut = 84;              // output side
constexpr int kMinIn = 2, kMaxIn = 512;  // accepted screen height / width

struct Axis {  // per output index: the two source indices and their weights
  float l0[kOut], l1[kOut];
  uint16_t i0[kOut], i1[kOut];
};

struct Tables {  // 3,040 B: passed to the kernel by value
  float v[256];
  Axis h, w;
};

inline void make_axis(Axis& ax, int in) {
  const float scale = (float)(in - 1) / (float)(kOut - 1);
  for (int d = 0; d < kOut; ++d) {
    const float src = scale * (float)d;
    int i0 = (int)src;
    if (i0 > in - 1) i0 = in - 1;
    const int i1 = i0 + 1 < in - 1 ? i0 + 1 : in - 1;
    float l1 = src - (float)i0;
    if (l1 > 1.0f) l1 = 1.0f;
    if (l1 < 0.0f) l1 = 0.0f;
    ax.l1[d] = l1;
    ax.l0[d] = 1.0f - l1;
    ax.i0[d] = (uint16_t)i0;
    ax.i1[d] = (uint16_t)i1;
  }
}

inline void make_tables(Tables& t, int height, int width) {
  for (int m = 0; m < 256; ++m) t.v[m] = (float)((double)m / 255.0);
  make_axis(t.h, height);
  make_axis(t.w, width);
}

// One output pixel.  r0 / r1: the element-wise max of the two screens along source rows i0h / i1h (RGB-interleaved);
// v: Tables::v.
RELA_ATARI_HD inline uint8_t feature_pixel(const float* v, const uint8_t* r0, const uint8_t* r1, int i0w, int i1w,
                                           float l0w, float l1w, float l0h, float l1h) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  float y[3];
  for (int c = 0; c < 3; ++c) {
    const float x00 = v[r0[3 * i0w + c]], x01 = v[r0[3 * i1w + c]];
    const float x10 = v[r1[3 * i0w + c]], x11 = v[r1[3 * i1w + c]];
    const float t0 = l0w * x00 + l1w * x01;
    const float t1 = l0w * x10 + l1w * x11;
    y[c] = l0h * t0 + l1h * t1;
  }
  const float g = (0.21f * y[0] + 0.72f * y[1]) + 0.07f * y[2];
  return (uint8_t)(g * 255.0f);
}

// Host restatement: a, b = [height][width][3] u8 (current, previous screen); out = [84][84] u8.
inline void host_features(const uint8_t* a, const uint8_t* b, int height, int width, uint8_t* out) {
  static thread_local Tables t;
  static thread_local int th = 0, tw = 0;
  if (th != height || tw != width) {
    make_tables(t, height, width);
    th = height;
    tw = width;
  }
  const int rb = width * 3;
  static thread_local uint8_t m[2][kMaxIn * 3];
  for (int y = 0; y < kOut; ++y) {
    const int src[2] = {t.h.i0[y], t.h.i1[y]};
    for (int k = 0; k < 2; ++k) {
      const uint8_t* pa = a + (int64_t)src[k] * rb;
      const uint8_t* pb = b + (int64_t)src[k] * rb;
      for (int i = 0; i < rb; ++i) m[k][i] = pa[i] > pb[i] ? pa[i] : pb[i];
    }
    for (int x = 0; x < kOut; ++x)
      out[y * kOut + x] = feature_pixel(t.v, m[0], m[1], t.w.i0[x], t.w.i1[x], t.w.l0[x], t.w.l1[x], t.h.l0[y], t.h.l1[y]);
  }
}

// Indexed-colour screens (ALEInterface::getScreen: one palette index per pixel): the frame computeFeature sees is, per
// channel, max(pal[ia][c], pal[ib][c]) -- the max is taken AFTER the lookup, as getScreenRGB followed by the recipe above
// does, so the features equal those of the expanded screens bit for bit.  All 256 indices are valid.
// One pixel of the max image: three bytes at dst from the indices ia / ib and pal = [256][3] u8 RGB.
RELA_ATARI_HD inline void indexed_max_pixel(const uint8_t* pal, uint8_t ia, uint8_t ib, uint8_t* dst) {
  for (int c = 0; c < 3; ++c) {
    const uint8_t a = pal[3 * ia + c], b = pal[3 * ib + c];
    dst[c] = a > b ? a : b;
  }
}

// Host restatement: ia, ib = [height][width] u8 indices (current, previous screen); pal = [256][3] u8; out = [84][84] u8.
inline void host_features_indexed(const uint8_t* ia, const uint8_t* ib, const uint8_t* pal, int height, int width,
                                  uint8_t* out) {
  static thread_local Tables t;
  static thread_local int th = 0, tw = 0;
  if (th != height || tw != width) {
    make_tables(t, height, width);
    th = height;
    tw = width;
  }
  static thread_local uint8_t m[2][kMaxIn * 3];
  for (int y = 0; y < kOut; ++y) {
    const int src[2] = {t.h.i0[y], t.h.i1[y]};
    for (int k = 0; k < 2; ++k) {
      const uint8_t* pa = ia + (int64_t)src[k] * width;
      const uint8_t* pb = ib + (int64_t)src[k] * width;
      for (int i = 0; i < width; ++i) indexed_max_pixel(pal, pa[i], pb[i], &m[k][3 * i]);
    }
    for (int x = 0; x < kOut; ++x)
      out[y * kOut + x] = feature_pixel(t.v, m[0], m[1], t.w.i0[x], t.w.i1[x], t.w.l0[x], t.w.l1[x], t.h.l0[y], t.h.l1[y]);
  }
}

}  // namespace rela_atari
