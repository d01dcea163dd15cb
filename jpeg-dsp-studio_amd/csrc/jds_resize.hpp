// jds_resize.hpp — Pillow's 8-bit Image.resize (ImagingResample: BOX, BILINEAR,
// HAMMING, BICUBIC, LANCZOS) on packed RGB (DESIGN.md "Pillow resizing";
// definition: tests/pillow_resize_ref.py).  Two parts:
//
//  * the coefficient builder, host only, in doubles and in Pillow's operation
//    order (precompute_coeffs + normalize_coeffs_8bpc): per output sample of an
//    axis its first input sample, its sample count and its 22-bit taps;
//  * the tile core of k_resize / k_resize_batch (jds_resize.hip), compiled for
//    host and device: the GPU lanes, the host tile loop behind
//    jds_selftest_resize and tools/resize_san.cpp run this same code.  All
//    pixel arithmetic is 32-bit.
//
// A tile is RS_TH output rows of at most RS_TW output columns and a lane owns
// one (column, channel) sample of every row.  The tile walks the input rows its
// output rows read, a few per step: the lanes stage the rows' segments (first
// input column of the tile's first output column to the last of its last) in
// LDS, each lane filters its sample of a staged row to a byte -- Pillow's uint8
// intermediate -- and adds it, times the vertical tap, to the accumulators of
// the output rows whose windows hold that input row.  The intermediate image is
// never written.  A pass Pillow skips passes the bytes through.
#pragma once
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include <vector>

#include "jds.h"

#pragma clang fp contract(off)

#ifndef JDS_HDI
#ifdef __HIPCC__
#define JDS_HDI __host__ __device__ __forceinline__
#else
#define JDS_HDI inline
#endif
#endif

namespace jds {

constexpr int RS_PB = 22;           // Pillow's PRECISION_BITS
constexpr int RS_NT = 192;          // lanes of a tile: RS_TW columns x 3 channels
constexpr int RS_TH = 16, RS_TW = 64;
constexpr int RS_HT_WORDS = 6144;   // LDS: the horizontal taps of a tile's columns
constexpr int RS_SEG_BYTES = 6144;  // LDS: the staged row segments; later the output rows
constexpr int RS_NR = 8;            // input rows staged per step, at most
constexpr int RS_OS = 200;          // bytes per staged output row (3 * RS_TW + 3 of phase, whole words)
// The tap cap: one output column's taps and segment must fit (RS_HT_WORDS
// words, RS_SEG_BYTES / 3 pixels); ksize is odd, and so is the cap.
constexpr int RS_MAX_TAPS = 1023;
static_assert(RS_NT == 3 * RS_TW && RS_MAX_TAPS <= RS_HT_WORDS && 3 * RS_MAX_TAPS + 6 <= RS_SEG_BYTES &&
                  RS_TH * RS_OS <= RS_SEG_BYTES && RS_OS % 4 == 0 && RS_OS >= RS_NT + 3,
              "tile");

// ------------------------------------------------ coefficients (host) --

inline double rs_f_box(double x) { return (x > -0.5 && x <= 0.5) ? 1.0 : 0.0; }
inline double rs_f_bilinear(double x) {
  if (x < 0.0) x = -x;
  return x < 1.0 ? 1.0 - x : 0.0;
}
inline double rs_f_hamming(double x) {
  if (x < 0.0) x = -x;
  if (x == 0.0) return 1.0;
  if (x >= 1.0) return 0.0;
  x = x * M_PI;
  return sin(x) / x * (0.54 + 0.46 * cos(x));
}
inline double rs_f_bicubic(double x) {
  const double a = -0.5;
  if (x < 0.0) x = -x;
  if (x < 1.0) return ((a + 2.0) * x - (a + 3.0)) * x * x + 1;
  if (x < 2.0) return (((x - 5) * x + 8) * x - 4) * a;
  return 0.0;
}
inline double rs_sinc(double x) {
  if (x == 0.0) return 1.0;
  x = x * M_PI;
  return sin(x) / x;
}
inline double rs_f_lanczos(double x) { return (-3.0 <= x && x < 3.0) ? rs_sinc(x) * rs_sinc(x / 3) : 0.0; }

inline bool rs_filter_ok(int flt) { return flt >= JDS_RESAMPLE_LANCZOS && flt <= JDS_RESAMPLE_HAMMING; }
inline double rs_filter_support(int flt) {
  return flt == JDS_RESAMPLE_LANCZOS ? 3.0 : flt == JDS_RESAMPLE_BICUBIC ? 2.0 : flt == JDS_RESAMPLE_BOX ? 0.5 : 1.0;
}
inline double rs_filter(int flt, double x) {
  switch (flt) {
    case JDS_RESAMPLE_LANCZOS: return rs_f_lanczos(x);
    case JDS_RESAMPLE_BILINEAR: return rs_f_bilinear(x);
    case JDS_RESAMPLE_BICUBIC: return rs_f_bicubic(x);
    case JDS_RESAMPLE_BOX: return rs_f_box(x);
    default: return rs_f_hamming(x);
  }
}

// The taps an axis needs per output sample (Pillow's ksize), as a double: the
// caller compares it with the cap before anything is sized by it.
inline double rs_ksize(float in0, float in1, int outSize, int flt) {
  const double scale = (double)(in1 - in0) / outSize;  // (the box edges are C floats, as their difference is)
  const double fs = scale < 1.0 ? 1.0 : scale;
  return ceil(rs_filter_support(flt) * fs) * 2 + 1;
}

// One axis' table: bounds[2 * xx] the first input sample of output sample xx,
// bounds[2 * xx + 1] their number, taps[xx * ksize + x] the fixed-point taps;
// worst: the largest 255 * sum|k| + 2^21 of a sample.
struct RsAxisTab {
  int ksize = 0;
  std::vector<int32_t> bounds, taps;
  long long worst = 0;
};

inline void rs_coeffs(int inSize, float in0f, float in1f, int outSize, int flt, RsAxisTab* t) {
  const double in0 = (double)in0f;
  const double scale = (double)(in1f - in0f) / outSize;
  const double fs = scale < 1.0 ? 1.0 : scale;
  const double support = rs_filter_support(flt) * fs;
  const int ksize = (int)ceil(support) * 2 + 1;
  t->ksize = ksize;
  t->bounds.assign(2 * (size_t)outSize, 0);
  t->taps.assign((size_t)outSize * (size_t)ksize, 0);
  t->worst = 0;
  std::vector<double> w((size_t)ksize);
  for (int xx = 0; xx < outSize; ++xx) {
    const double center = in0 + (xx + 0.5) * scale;
    const double ss = 1.0 / fs;
    int xmin = (int)(center - support + 0.5);
    if (xmin < 0) xmin = 0;
    int xmax = (int)(center + support + 0.5);
    if (xmax > inSize) xmax = inSize;
    xmax -= xmin;
    double ww = 0.0;
    for (int x = 0; x < xmax; ++x) {
      w[(size_t)x] = rs_filter(flt, (x + xmin - center + 0.5) * ss);
      ww += w[(size_t)x];
    }
    long long sum = 0;
    for (int x = 0; x < xmax; ++x) {
      double v = w[(size_t)x];
      if (ww != 0.0) v /= ww;
      const int32_t k = v < 0 ? (int32_t)(-0.5 + v * (1 << RS_PB)) : (int32_t)(0.5 + v * (1 << RS_PB));
      t->taps[(size_t)xx * (size_t)ksize + (size_t)x] = k;
      sum += k < 0 ? -(long long)k : (long long)k;
    }
    const long long worst = 255 * sum + (1ll << (RS_PB - 1));
    if (worst > t->worst) t->worst = worst;
    t->bounds[2 * (size_t)xx] = xmin;
    t->bounds[2 * (size_t)xx + 1] = xmax;
  }
}

// ------------------------------------------------------ launch records --

// One resize of one image: uniform over its tiles.  Offsets hb .. vt count
// int32 words from the table base (hb, vb: bounds; ht, vt: taps); src_off /
// dst_off bytes from the source / destination base chosen by src_sel / dst_sel.
struct RsRec {
  long long src_off, dst_off;
  long long hb, ht, vb, vt;
  int H, W, oh, ow;
  int ksh, ksv, needh, needv;
  int tw, nr, segs;      // the image's tile width, rows staged per step, LDS bytes per staged row
  int tiles_x, tiles_y;
  int st;                // index of the status word that zeroes the slot when set, or -1
  int zero;              // the slot is zeros whatever the status says (a file that did not parse)
  int src_sel, dst_sel;  // 0: the caller's buffer; 1: the scratch of the tall-image rule
  int pad_;
};

struct RsMap {
  int tile0;  // the record's first tile in the launch (sentinel: the launch's tiles)
  int rec;
};

JDS_HDI int rs_find(const RsMap* map, int n, int t) {
  int lo = 0, hi = n;
  while (hi - lo > 1) {
    const int mid = lo + (hi - lo) / 2;
    if (map[mid].tile0 <= t)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

// Image.resize's rule: a very tall image that shrinks is resized vertically first.
inline bool rs_tall(long long H, long long W, long long oh) { return H > W * 100 && oh < H; }

// RS_E*: what a plan can refuse; the message goes to err.
constexpr int RS_EINVAL = 1, RS_ENOTSUP = 2;

inline int rs_check_box(long long H, long long W, const float* box, char* err, size_t errn) {
  if (!(box[0] >= 0.0f && box[1] >= 0.0f && box[2] <= (float)W && box[3] <= (float)H && box[0] < box[2] &&
        box[1] < box[3])) {
    snprintf(err, errn, "box (%g, %g, %g, %g) is empty or not within the %lld x %lld image", (double)box[0],
             (double)box[1], (double)box[2], (double)box[3], W, H);
    return RS_EINVAL;
  }
  return 0;
}

// The plan of one ImagingResample call: both axes' tables appended to `words`,
// the record's geometry, tile width and staging filled in (src_off, dst_off,
// st, zero, *_sel are the caller's).  worst (nullable): raised to the largest
// accumulator bound of the tables built.
inline int rs_plan(long long H, long long W, const float* box, long long oh, long long ow, int flt,
                   std::vector<int32_t>& words, RsRec* r, long long* worst, char* err, size_t errn) {
  if (!rs_filter_ok(flt)) {
    snprintf(err, errn, "unknown resampling filter %d: 1 LANCZOS, 2 BILINEAR, 3 BICUBIC, 4 BOX, 5 HAMMING", flt);
    return RS_EINVAL;
  }
  if (H < 1 || W < 1 || oh < 1 || ow < 1) {
    snprintf(err, errn, "bad size: %lld x %lld to %lld x %lld (width x height)", W, H, ow, oh);
    return RS_EINVAL;
  }
  if (int rc = rs_check_box(H, W, box, err, errn)) return rc;
  if (H > 0x7fffffffll / 3 || W > 0x7fffffffll / 3 || oh > 0x7fffffffll / 3 || ow > 0x7fffffffll / 3 ||
      oh * ow * 3 > 0x7fffffffll || H * W * 3 > 0x7fffffffll) {
    snprintf(err, errn, "image too large: more than 2^31 - 1 bytes");
    return RS_ENOTSUP;
  }
  r->H = (int)H;
  r->W = (int)W;
  r->oh = (int)oh;
  r->ow = (int)ow;
  r->needh = (ow != W || box[0] != 0.0f || box[2] != (float)W) ? 1 : 0;
  r->needv = (oh != H || box[1] != 0.0f || box[3] != (float)H) ? 1 : 0;
  r->ksh = r->ksv = 0;
  r->hb = r->ht = r->vb = r->vt = 0;
  for (int ax = 0; ax < 2; ++ax) {
    if (!(ax ? r->needv : r->needh)) continue;
    const float in0 = box[ax], in1 = box[2 + ax];
    const int outSize = ax ? r->oh : r->ow, inSize = ax ? r->H : r->W;
    const double ks = rs_ksize(in0, in1, outSize, flt);
    if (ks > (double)RS_MAX_TAPS) {
      snprintf(err, errn, "%s axis needs %.0f taps per output sample, the kernel's cap is %d",
               ax ? "vertical" : "horizontal", ks, RS_MAX_TAPS);
      return RS_ENOTSUP;
    }
    RsAxisTab t;
    rs_coeffs(inSize, in0, in1, outSize, flt, &t);
    if (t.worst > 0x7fffffffll) {
      snprintf(err, errn, "%s axis: a 32-bit accumulator could reach %lld", ax ? "vertical" : "horizontal", t.worst);
      return RS_ENOTSUP;
    }
    if (worst && t.worst > *worst) *worst = t.worst;
    const long long b = (long long)words.size();
    words.insert(words.end(), t.bounds.begin(), t.bounds.end());
    const long long k = (long long)words.size();
    words.insert(words.end(), t.taps.begin(), t.taps.end());
    if (ax) {
      r->ksv = t.ksize;
      r->vb = b;
      r->vt = k;
    } else {
      r->ksh = t.ksize;
      r->hb = b;
      r->ht = k;
    }
  }
  // the tile width: the columns' taps in RS_HT_WORDS, every tile's segment in RS_SEG_BYTES
  int tw = r->ow < RS_TW ? r->ow : RS_TW;
  int maxlen = tw;
  if (r->needh) {
    if (tw > RS_HT_WORDS / r->ksh) tw = RS_HT_WORDS / r->ksh;
    const int32_t* hb = words.data() + r->hb;
    for (;; --tw) {
      maxlen = 0;
      for (int x0 = 0; x0 < r->ow; x0 += tw) {
        const int xl = (x0 + tw < r->ow ? x0 + tw : r->ow) - 1;
        const int len = hb[2 * xl] + hb[2 * xl + 1] - hb[2 * x0];
        if (len > maxlen) maxlen = len;
      }
      if (3 * maxlen + 6 <= RS_SEG_BYTES || tw == 1) break;
    }
  }
  r->tw = tw;
  r->segs = (3 * maxlen + 6) & ~3;
  r->nr = RS_SEG_BYTES / r->segs < RS_NR ? RS_SEG_BYTES / r->segs : RS_NR;
  r->tiles_x = (r->ow + tw - 1) / tw;
  r->tiles_y = (r->oh + RS_TH - 1) / RS_TH;
  if ((long long)r->tiles_x * r->tiles_y > 0x7fffffffll) {
    snprintf(err, errn, "image too large: more than 2^31 - 1 tiles");
    return RS_ENOTSUP;
  }
  r->pad_ = 0;
  return 0;
}

// ------------------------------------------------------------ tile core --

struct RsShared {
  int32_t ht[RS_HT_WORDS];
  alignas(4) uint8_t seg[RS_SEG_BYTES];
};

// A tile: its output pixels, the input columns [xs, xe) its rows' segments hold
// and the input rows [ys, ye) it walks.
struct RsTile {
  int X0, Y0, nc, nrw, xs, xe, ys, ye;
};

JDS_HDI RsTile rs_tile(const RsRec& r, const int32_t* tabs, int ty, int tx) {
  RsTile t;
  t.X0 = tx * r.tw;
  t.Y0 = ty * RS_TH;
  t.nc = (t.X0 + r.tw < r.ow ? t.X0 + r.tw : r.ow) - t.X0;
  t.nrw = (t.Y0 + RS_TH < r.oh ? t.Y0 + RS_TH : r.oh) - t.Y0;
  if (r.needh) {
    const int32_t* hb = tabs + r.hb;
    const int xl = t.X0 + t.nc - 1;
    t.xs = hb[2 * t.X0];
    t.xe = hb[2 * xl] + hb[2 * xl + 1];
  } else {
    t.xs = t.X0;
    t.xe = t.X0 + t.nc;
  }
  if (r.needv) {
    const int32_t* vb = tabs + r.vb;
    const int yl = t.Y0 + t.nrw - 1;
    t.ys = vb[2 * t.Y0];
    t.ye = vb[2 * yl] + vb[2 * yl + 1];
  } else {
    t.ys = t.Y0;
    t.ye = t.Y0 + t.nrw;
  }
  return t;
}

JDS_HDI int rs_phase(const uint8_t* p) { return (int)((uintptr_t)p & 3u); }

// Lane i of nt: n bytes from g (any alignment) into the slot, byte j at
// slot[phase + j], so that whole aligned words of the source are whole aligned
// words of the slot.  Words inside [g, g + n) are loaded as words, the ragged
// ends as bytes: nothing outside is read.  e counts words over `rows` rows of
// ndw words each (row q's bytes start at g + q * pitch, its slot at slot + q * segs).
JDS_HDI void rs_stage_lane(uint8_t* slot, int segs, const uint8_t* g, long long pitch, int n, int rows, int i,
                           int nt) {
  const int ndw = segs >> 2;
  for (int e = i; e < rows * ndw; e += nt) {
    const int q = e / ndw, d = e - q * ndw;
    const uint8_t* gq = g + (long long)q * pitch;
    const int j = 4 * d - rs_phase(gq);
    uint8_t* o = slot + q * segs + 4 * d;
    if (j >= 0 && j + 4 <= n) {
      uint32_t v;
      __builtin_memcpy(&v, __builtin_assume_aligned(gq + j, 4), 4);
      __builtin_memcpy(__builtin_assume_aligned(o, 4), &v, 4);
    } else {
      for (int b = 0; b < 4; ++b)
        if (j + b >= 0 && j + b < n) o[b] = gq[j + b];
    }
  }
}

// The mirror: n bytes per row from the slots to g; words where the address
// allows, bytes at the ragged ends; nothing outside [g, g + n) is written.
JDS_HDI void rs_store_lane(const uint8_t* slot, int segs, uint8_t* g, long long pitch, int n, int rows, int i,
                           int nt) {
  const int ndw = segs >> 2;
  for (int e = i; e < rows * ndw; e += nt) {
    const int q = e / ndw, d = e - q * ndw;
    uint8_t* gq = g + (long long)q * pitch;
    const int j = 4 * d - rs_phase(gq);
    const uint8_t* s = slot + q * segs + 4 * d;
    if (j >= 0 && j + 4 <= n) {
      uint32_t v;
      __builtin_memcpy(&v, __builtin_assume_aligned(s, 4), 4);
      __builtin_memcpy(__builtin_assume_aligned(gq + j, 4), &v, 4);
    } else {
      for (int b = 0; b < 4; ++b)
        if (j + b >= 0 && j + b < n) gq[j + b] = s[b];
    }
  }
}

JDS_HDI int rs_clip8(int32_t s) {
  const int32_t v = s >> RS_PB;  // (arithmetic)
  return v < 0 ? 0 : v > 255 ? 255 : v;
}

// What a lane keeps of its column: where its first sample lies in a staged row
// (bytes after the segment's first), its sample count and its taps in sh.ht.
struct RsCol {
  int xo, xn, tap0;
};

JDS_HDI RsCol rs_col(const RsRec& r, const int32_t* tabs, const RsTile& t, int c, int ch) {
  RsCol k;
  if (r.needh) {
    const int32_t* hb = tabs + r.hb + 2 * (t.X0 + c);
    k.xo = 3 * (hb[0] - t.xs) + ch;
    k.xn = hb[1];
  } else {
    k.xo = 3 * c + ch;
    k.xn = 1;
  }
  k.tap0 = c * r.ksh;
  return k;
}

// The lane's sample of a staged row (row: the segment's first byte): the
// horizontal pass and its rounding to a byte, or the byte itself.
JDS_HDI int rs_hsample(const RsShared& sh, const uint8_t* row, const RsCol& k, bool needh) {
  if (!needh) return row[k.xo];
  int32_t s = 1 << (RS_PB - 1);
  const int32_t* tp = sh.ht + k.tap0;
  const uint8_t* px = row + k.xo;
  for (int x = 0; x < k.xn; ++x) s += (int32_t)px[3 * x] * tp[x];
  return rs_clip8(s);
}

// The output rows' windows of a tile (uniform): ya[r] the first input row of
// output row Y0 + r, yn[r] their number (0 beyond the tile).
JDS_HDI void rs_windows(const RsRec& r, const int32_t* tabs, const RsTile& t, int (&ya)[RS_TH], int (&yn)[RS_TH]) {
  for (int i = 0; i < RS_TH; ++i) {
    if (i >= t.nrw) {
      ya[i] = 0;
      yn[i] = 0;
    } else if (r.needv) {
      ya[i] = tabs[r.vb + 2 * (t.Y0 + i)];
      yn[i] = tabs[r.vb + 2 * (t.Y0 + i) + 1];
    } else {
      ya[i] = t.Y0 + i;
      yn[i] = 1;
    }
  }
}

JDS_HDI void rs_acc_init(const RsRec& r, int32_t (&acc)[RS_TH]) {
  for (int i = 0; i < RS_TH; ++i) acc[i] = r.needv ? 1 << (RS_PB - 1) : 0;
}

// Input row y's byte b into the accumulators of the rows whose windows hold y.
JDS_HDI void rs_vacc(const RsRec& r, const int32_t* tabs, const RsTile& t, const int (&ya)[RS_TH],
                     const int (&yn)[RS_TH], int y, int b, int32_t (&acc)[RS_TH]) {
#pragma unroll
  for (int i = 0; i < RS_TH; ++i) {
    const int d = y - ya[i];
    if ((unsigned)d < (unsigned)yn[i])
      acc[i] += r.needv ? b * tabs[r.vt + (long long)(t.Y0 + i) * r.ksv + d] : b;
  }
}

// The tile's destination rows: first byte and pitch.
JDS_HDI uint8_t* rs_dst(const RsRec& r, const RsTile& t, uint8_t* dst) {
  return dst + ((long long)t.Y0 * r.ow + t.X0) * 3;
}

// The vertical pass' rounding: the accumulators become the output bytes.
JDS_HDI void rs_finish(const RsRec& r, int32_t (&acc)[RS_TH]) {
#pragma unroll
  for (int i = 0; i < RS_TH; ++i)
    if (r.needv) acc[i] = rs_clip8(acc[i]);
}

// A lane's finished bytes into the output staging rows (sh.seg, reused).
JDS_HDI void rs_emit(RsShared& sh, const RsRec& r, const RsTile& t, uint8_t* dst, int s, const int32_t (&acc)[RS_TH]) {
  uint8_t* g = rs_dst(r, t, dst);
#pragma unroll
  for (int i = 0; i < RS_TH; ++i)
    if (i < t.nrw) sh.seg[i * RS_OS + rs_phase(g + (long long)i * r.ow * 3) + s] = (uint8_t)acc[i];
}

struct RsAcc {
  int32_t a[RS_TH];
};

// One tile on the host: the kernel's steps with loops in place of lanes and of
// the barriers between them.  zero: the slot's bytes are zeros.
inline void rs_host_tile(RsShared& sh, const RsRec& r, const int32_t* tabs, const uint8_t* src, uint8_t* dst, int ty,
                         int tx, bool zero) {
  const RsTile t = rs_tile(r, tabs, ty, tx);
  static thread_local RsAcc accs[RS_NT];  // (a lane's are set before they are read)
  auto acc_of = [&](int s) -> int32_t(&)[RS_TH] { return accs[s].a; };
  if (!zero) {
    if (r.needh)
      for (int e = 0; e < t.nc * r.ksh; ++e) sh.ht[e] = tabs[r.ht + (long long)t.X0 * r.ksh + e];
    int ya[RS_TH], yn[RS_TH];
    rs_windows(r, tabs, t, ya, yn);
    for (int s = 0; s < 3 * t.nc; ++s) rs_acc_init(r, acc_of(s));
    const int n = 3 * (t.xe - t.xs);
    for (int y = t.ys; y < t.ye; y += r.nr) {
      const int rows = t.ye - y < r.nr ? t.ye - y : r.nr;
      const uint8_t* g = src + ((long long)y * r.W + t.xs) * 3;
      for (int i = 0; i < RS_NT && i < rows * (r.segs >> 2); ++i)  // (the lanes beyond have no word)
        rs_stage_lane(sh.seg, r.segs, g, (long long)r.W * 3, n, rows, i, RS_NT);
      for (int s = 0; s < 3 * t.nc; ++s) {
        const RsCol k = rs_col(r, tabs, t, s / 3, s % 3);
        for (int q = 0; q < rows; ++q) {
          const uint8_t* row = sh.seg + q * r.segs + rs_phase(g + (long long)q * r.W * 3);
          rs_vacc(r, tabs, t, ya, yn, y + q, rs_hsample(sh, row, k, r.needh != 0), acc_of(s));
        }
      }
    }
    for (int s = 0; s < 3 * t.nc; ++s) rs_finish(r, acc_of(s));
  } else {
    for (int s = 0; s < 3 * t.nc; ++s) memset(acc_of(s), 0, sizeof(RsAcc));
  }
  for (int s = 0; s < 3 * t.nc; ++s) rs_emit(sh, r, t, dst, s, acc_of(s));
  for (int i = 0; i < RS_NT; ++i)
    rs_store_lane(sh.seg, RS_OS, rs_dst(r, t, dst), (long long)r.ow * 3, 3 * t.nc, t.nrw, i, RS_NT);
}

// The host tile loop of one record.
inline void rs_host_image(const RsRec& r, const int32_t* tabs, const uint8_t* src, uint8_t* dst, bool zero) {
  static thread_local RsShared sh;  // (what a step reads of it, the step before has written)
  for (int ty = 0; ty < r.tiles_y; ++ty)
    for (int tx = 0; tx < r.tiles_x; ++tx) rs_host_tile(sh, r, tabs, src, dst, ty, tx, zero);
}

// Image.resize on the host: the tall-image rule around one or two plans, each
// run by the host tile loop.  worst: as rs_plan's.
inline int rs_host_resize(const uint8_t* src, long long H, long long W, const float* box_in, long long oh, long long ow,
                          int flt, uint8_t* dst, long long* worst, char* err, size_t errn) {
  const float full[4] = {0.0f, 0.0f, (float)W, (float)H};
  const float* box = box_in ? box_in : full;
  std::vector<int32_t> words;
  RsRec r;
  memset(&r, 0, sizeof r);
  r.st = -1;
  if (H >= 1 && W >= 1 && oh >= 1 && ow >= 1 && rs_filter_ok(flt) && !rs_check_box(H, W, box, err, errn) &&
      rs_tall(H, W, oh)) {
    const float b1[4] = {0.0f, box[1], (float)W, box[3]}, b2[4] = {box[0], 0.0f, box[2], (float)oh};
    if (int rc = rs_plan(H, W, b1, oh, W, flt, words, &r, worst, err, errn)) return rc;
    std::vector<uint8_t> mid((size_t)oh * (size_t)W * 3);
    rs_host_image(r, words.data(), src, mid.data(), false);
    words.clear();
    if (int rc = rs_plan(oh, W, b2, oh, ow, flt, words, &r, worst, err, errn)) return rc;
    rs_host_image(r, words.data(), mid.data(), dst, false);
    return 0;
  }
  if (int rc = rs_plan(H, W, box, oh, ow, flt, words, &r, worst, err, errn)) return rc;
  rs_host_image(r, words.data(), src, dst, false);
  return 0;
}

}  // namespace jds
