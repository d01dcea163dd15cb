// jpeg_ljs_san.cpp — stand-alone host program over the tile core of the scaled
// libjpeg rendering (csrc/jds_jpeg_ljs.hpp, DESIGN.md "Scaled libjpeg
// rendering"), for sanitizer runs:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ijpeg-dsp-studio_amd/csrc tools/jpeg_ljs_san.cpp -o jpeg_ljs_san
//   ./jpeg_ljs_san
//
// Runs the host tile loop (jpeg_ljs_host_image: the kernel's own expressions)
// in 4:4:4, 4:2:2, 4:2:0 and grayscale at 1/2, 1/4 and 1/8 over every size up
// to 40 x 40 and over sizes around one, two and three tiles on each axis, from
// heap arrays of exactly coeffs_needed entries and out_h*out_w*3 bytes, and
// compares every byte with a plain whole-plane implementation of the rules
// below (int64 values reduced to 32 bits where the core's are: reduced planes,
// cropped, then upsampling, then colour; no tiles, no window, no staging).  The
// coefficients rotate through sparse ordinary blocks, dense saturating ones and
// full-range int16 (+-32767 and -32768 everywhere) with every table entry 255,
// where the 32-bit arithmetic wraps.  A batch of all four modes with mixed
// denominators (1 among them) and one flagged image goes through the batch
// model.  No HIP, no GPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jds_jpeg_ljs.hpp"

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

static long g_images = 0, g_checks = 0, g_failed = 0;
#define CHECK(cond, ...)                      \
  do {                                        \
    ++g_checks;                               \
    if (!(cond)) {                            \
      ++g_failed;                             \
      fprintf(stderr, "FAILED: %s: ", #cond); \
      fprintf(stderr, __VA_ARGS__);           \
      fprintf(stderr, "\n");                  \
    }                                         \
  } while (0)

// ------------------------------------------------- the plain implementation --
static int64_t w32(int64_t x) { return (int64_t)(int32_t)(uint32_t)(uint64_t)x; }
static int64_t dsc(int64_t x, int n) { return w32(x + ((int64_t)1 << (n - 1))) >> n; }

// one n-point pass (n = 4 or 2) over 8 inputs `stride` apart, outputs DESCALEd by sh
static void pass(const int64_t* in, int stride, int64_t* out, int ostride, int n, int sh) {
  int64_t i[8];
  for (int k = 0; k < 8; ++k) i[k] = w32(in[k * stride]);
  if (n == 4) {
    const int64_t t0 = i[0] * 16384, t2 = 15137 * i[2] - 6270 * i[6], t10 = t0 + t2, t12 = t0 - t2;
    const int64_t a = -1730 * i[7] + 11893 * i[5] - 17799 * i[3] + 8697 * i[1];
    const int64_t b = -4176 * i[7] - 4926 * i[5] + 7373 * i[3] + 20995 * i[1];
    const int64_t o[4] = {t10 + b, t12 + a, t12 - a, t10 - b};
    for (int k = 0; k < 4; ++k) out[k * ostride] = dsc(w32(o[k]), sh);
  } else {
    const int64_t t10 = i[0] * 32768, t = -5906 * i[7] + 6967 * i[5] - 10426 * i[3] + 29692 * i[1];
    out[0] = dsc(w32(t10 + t), sh);
    out[ostride] = dsc(w32(t10 - t), sh);
  }
}

// the 8-point pass of the full-scale rendering (4:2:0 chroma at 1/2)
static void pass8(const int64_t* in, int stride, int64_t* out, int ostride, int n) {
  int64_t i[8];
  for (int k = 0; k < 8; ++k) i[k] = w32(in[k * stride]);
  int64_t z1 = (i[2] + i[6]) * 4433, tmp2 = z1 - i[6] * 15137, tmp3 = z1 + i[2] * 6270;
  const int64_t tmp0 = (i[0] + i[4]) * 8192, tmp1 = (i[0] - i[4]) * 8192;
  const int64_t t10 = tmp0 + tmp3, t13 = tmp0 - tmp3, t11 = tmp1 + tmp2, t12 = tmp1 - tmp2;
  int64_t a0 = i[7], a1 = i[5], a2 = i[3], a3 = i[1];
  z1 = a0 + a3;
  int64_t z2 = a1 + a2, z3 = a0 + a2, z4 = a1 + a3;
  const int64_t z5 = (z3 + z4) * 9633;
  a0 *= 2446, a1 *= 16819, a2 *= 25172, a3 *= 12299;
  z1 *= -7373, z2 *= -20995, z3 = z3 * -16069 + z5, z4 = z4 * -3196 + z5;
  a0 += z1 + z3, a1 += z2 + z4, a2 += z2 + z3, a3 += z1 + z4;
  const int64_t o[8] = {t10 + a3, t11 + a2, t12 + a1, t13 + a0, t13 - a0, t12 - a1, t11 - a2, t10 - a3};
  for (int k = 0; k < 8; ++k) out[k * ostride] = dsc(w32(o[k]), n);
}

// gr x gc blocks through the size-point inverse -> the h x w plane of samples in [0, 255]
static std::vector<int> plane_of(const int16_t* cf, const int* q, int gr, int gc, int size, int h, int w) {
  std::vector<int> p((size_t)h * w);
  for (int by = 0; by < gr; ++by)
    for (int bx = 0; bx < gc; ++bx) {
      const int16_t* b = cf + ((size_t)by * gc + bx) * 64;
      int64_t d[64], ws[64] = {0}, px[64] = {0};
      for (int i = 0; i < 64; ++i) d[i] = (int64_t)b[i] * q[i];
      if (size == 8) {
        for (int c = 0; c < 8; ++c) pass8(d + c, 8, ws + c, 8, 11);
        for (int r = 0; r < 8; ++r) pass8(ws + 8 * r, 1, px + 8 * r, 1, 18);
      } else if (size == 1) {
        px[0] = dsc(w32(d[0]), 3);
      } else {
        for (int c = 0; c < 8; ++c) pass(d + c, 8, ws + c, 8, size, size == 4 ? 12 : 13);
        for (int r = 0; r < size; ++r) pass(ws + 8 * r, 1, px + 8 * r, 1, size, size == 4 ? 19 : 20);
      }
      for (int r = 0; r < size; ++r)
        for (int c = 0; c < size; ++c) {
          const int y = by * size + r, x = bx * size + c;
          if (y >= h || x >= w) continue;
          const int64_t s = w32(px[8 * r + c] + 128);
          p[(size_t)y * w + x] = (int)(s < 0 ? 0 : s > 255 ? 255 : s);
        }
    }
  return p;
}

static int at(const std::vector<int>& p, int h, int w, int y, int x) {
  y = y < 0 ? 0 : y >= h ? h - 1 : y;
  x = x < 0 ? 0 : x >= w ? w - 1 : x;
  return p[(size_t)y * w + x];
}

// the chroma sample under pixel (y, x): none left to upsample (ux == 1), or h2v1 with
// the fancy taps when m > 1 and the plane is more than two samples wide
static int chroma_at(const std::vector<int>& p, int ch, int cw, int ux, int m, int y, int x) {
  if (ux == 1) return at(p, ch, cw, y, x);
  const int cx = x / 2;
  if (m == 1 || cw <= 2) return at(p, ch, cw, y, cx);
  const int nx = (x & 1) ? cx + 1 : cx - 1;
  return (3 * at(p, ch, cw, y, cx) + at(p, ch, cw, y, nx) + ((x & 1) ? 2 : 1)) >> 2;
}

static uint8_t clamp8(int v) { return (uint8_t)(v < 0 ? 0 : v > 255 ? 255 : v); }

static int chroma_size(int m, int hmax, int vmax) {
  int s = m;
  while (s < 8 && (hmax * m) % (2 * s) == 0 && (vmax * m) % (2 * s) == 0) s *= 2;
  return s;
}

static void plain_render(const jds::JInvArgs& a, int denom, const int16_t* cf, uint8_t* rgb) {
  const int m = 8 / denom, oh = (a.H + denom - 1) / denom, ow = (a.W + denom - 1) / denom;
  const std::vector<int> Y = plane_of(cf + a.off[0], a.q[0], a.gr[0], a.gc[0], m, oh, ow);
  if (a.ss == JDS_SS_GRAY) {
    for (size_t i = 0; i < Y.size(); ++i) rgb[3 * i] = rgb[3 * i + 1] = rgb[3 * i + 2] = (uint8_t)Y[i];
    return;
  }
  const int vmax = a.ss == JDS_SS_420 ? 2 : 1, hmax = a.ss == JDS_SS_444 ? 1 : 2;
  const int s = chroma_size(m, hmax, vmax), ux = hmax * m / s;
  const int ch = (a.H * s + 8 * vmax - 1) / (8 * vmax), cw = (a.W * s + 8 * hmax - 1) / (8 * hmax);
  CHECK(vmax * m / s == 1 && (ux == 1 || ux == 2), "upsampling factors");
  const std::vector<int> Cb = plane_of(cf + a.off[1], a.q[1], a.gr[1], a.gc[1], s, ch, cw);
  const std::vector<int> Cr = plane_of(cf + a.off[2], a.q[2], a.gr[2], a.gc[2], s, ch, cw);
  for (int y = 0; y < oh; ++y)
    for (int x = 0; x < ow; ++x) {
      const int yy = Y[(size_t)y * ow + x], cb = chroma_at(Cb, ch, cw, ux, m, y, x) - 128,
                cr = chroma_at(Cr, ch, cw, ux, m, y, x) - 128;
      uint8_t* o = rgb + ((size_t)y * ow + x) * 3;
      o[0] = clamp8(yy + ((91881 * cr + 32768) >> 16));
      o[1] = clamp8(yy + ((-22554 * cb - 46802 * cr + 32768) >> 16));
      o[2] = clamp8(yy + ((116130 * cb + 32768) >> 16));
    }
}

// ------------------------------------------------------------------ inputs --
static void fill_info(jds_jpeg_info* info, int H, int W, int ss, int qkind) {
  memset(info, 0, sizeof *info);
  info->H = H;
  info->W = W;
  info->subsampling = ss;
  const int vmax = ss == JDS_SS_420 ? 2 : 1, hmax = (ss == JDS_SS_420 || ss == JDS_SS_422) ? 2 : 1;
  long long need = 0;
  for (int c = 0; c < (ss == JDS_SS_GRAY ? 1 : 3); ++c) {
    const int h = c ? (H + vmax - 1) / vmax : H, w = c ? (W + hmax - 1) / hmax : W;
    info->grid_rows[c] = (h + 7) / 8;
    info->grid_cols[c] = (w + 7) / 8;
    need += 64ll * info->grid_rows[c] * info->grid_cols[c];
    for (int i = 0; i < 64; ++i) info->qtable[c][i] = qkind == 1 ? 255.0 : (double)(1 + (rnd() % (qkind ? 255 : 24)));
  }
  info->coeffs_needed = need;
}

// kind 0: sparse ordinary blocks; 1: full-range int16; 2: dense, saturating both ends
static void fill_coeffs(std::vector<int16_t>& cf, int kind) {
  for (size_t i = 0; i < cf.size(); ++i) {
    const uint32_t r = rnd();
    if (kind == 1)
      cf[i] = (int16_t)((r % 3) == 0 ? -32768 : (r % 3) == 1 ? 32767 : -32767);
    else if (kind == 2)
      cf[i] = (int16_t)((int)(r % 601) - 300);
    else if (i % 64 == 0)
      cf[i] = (int16_t)((int)(r % 401) - 200);
    else
      cf[i] = (int16_t)((r & 3) ? 0 : (int)((r >> 2) % 81) - 40);
  }
}

static void one_image(int H, int W, int ss, int kind) {
  jds_jpeg_info info;
  fill_info(&info, H, W, ss, kind);
  jds::JInvArgs a;
  const int rc = jds::jinv_args(&info, &a);
  CHECK(rc == 0, "jinv_args %dx%d mode %d: %d", H, W, ss, rc);
  if (rc) return;
  std::vector<int16_t> cf((size_t)info.coeffs_needed);
  fill_coeffs(cf, kind);
  for (int denom = 2; denom <= 8; denom *= 2) {
    long long oh, ow;
    jds::ls_scaled_size(H, W, denom, &oh, &ow);
    std::vector<uint8_t> got((size_t)(oh * ow * 3), 0x5a), exp((size_t)(oh * ow * 3), 0xa5);
    jds::jpeg_ljs_host_image(a, denom, cf.data(), got.data());
    plain_render(a, denom, cf.data(), exp.data());
    CHECK(got == exp, "%dx%d mode %d kind %d denominator %d differs", H, W, ss, kind, denom);
    ++g_images;
  }
}

static void one_batch() {
  const int N = 9;
  const int sizes[N][4] = {{37, 53, JDS_SS_420, 2},  {9, 9, JDS_SS_444, 4},    {33, 130, JDS_SS_422, 2},
                           {40, 136, JDS_SS_GRAY, 8}, {65, 257, JDS_SS_420, 8}, {65, 257, JDS_SS_420, 1},
                           {33, 130, JDS_SS_422, 4},  {3, 5, JDS_SS_444, 8},    {37, 53, JDS_SS_420, 2}};
  std::vector<jds::JInvRec> recs(N);
  std::vector<int16_t> cf;
  long long rb = 0, ce = 0;
  for (int k = 0; k < N; ++k) {
    jds_jpeg_info info;
    fill_info(&info, sizes[k][0], sizes[k][1], sizes[k][2], 0);
    memset(&recs[k], 0, sizeof recs[k]);
    CHECK(jds::jinv_args(&info, &recs[k].a) == 0, "batch args %d", k);
    jds::ls_batch_place(recs[k], k, sizes[k][3], info.coeffs_needed, &rb, &ce);
    CHECK(recs[k].rgb_off % jds::JI_RGB_ALIGN == 0 && jds::ls_rec_denom(recs[k]) == sizes[k][3], "placement %d", k);
  }
  cf.resize((size_t)ce);
  fill_coeffs(cf, 2);
  std::vector<jds::JInvMap> map[jds::JI_MODES], smap[jds::JI_MODES][jds::LS_ND];
  CHECK(jds::ls_batch_maps(recs.data(), N, map, smap), "maps");
  const jds::JInvMap* mp[jds::JI_MODES];
  const jds::JInvMap* smp[jds::JI_MODES][jds::LS_ND];
  int nmap[jds::JI_MODES], nsmap[jds::JI_MODES][jds::LS_ND];
  for (int m = 0; m < jds::JI_MODES; ++m) {
    mp[m] = map[m].data();
    nmap[m] = (int)map[m].size() - 1;
    for (int d = 0; d < jds::LS_ND; ++d) {
      smp[m][d] = smap[m][d].data();
      nsmap[m][d] = (int)smap[m][d].size() - 1;
    }
  }
  CHECK(nmap[JDS_SS_420] == 1 && nsmap[JDS_SS_420][0] == 2 && nsmap[JDS_SS_422][1] == 1, "map sizes");
  std::vector<uint32_t> st(N, 0u);
  st[2] = 4u;  // the first 4:2:2 image's scan was defective
  std::vector<uint8_t> rgb((size_t)rb, 0xa5);
  jds::jpeg_ljt_batch_host(recs.data(), mp, nmap, st.data(), cf.data(), rgb.data());
  jds::jpeg_ljs_batch_host(recs.data(), smp, nsmap, st.data(), cf.data(), rgb.data());
  for (int k = 0; k < N; ++k) {
    const jds::JInvRec& r = recs[k];
    long long oh, ow;
    jds::ls_scaled_size(r.a.H, r.a.W, sizes[k][3], &oh, &ow);
    const size_t n = (size_t)(oh * ow * 3);
    std::vector<uint8_t> exp(n, 0);
    if (!st[k]) {
      if (sizes[k][3] == 1)
        jds::jpeg_ljt_host_image(r.a, cf.data() + r.coef_off, exp.data());
      else
        plain_render(r.a, sizes[k][3], cf.data() + r.coef_off, exp.data());
    }
    CHECK(memcmp(rgb.data() + r.rgb_off, exp.data(), n) == 0, "batch image %d", k);
    const size_t end = (size_t)r.rgb_off + n, next = k + 1 < N ? (size_t)recs[k + 1].rgb_off : (size_t)rb;
    bool gap = true;
    for (size_t i = end; i < next; ++i) gap = gap && rgb[i] == 0xa5;
    CHECK(gap, "bytes behind batch image %d were written", k);
    ++g_images;
  }
}

int main() {
  const int modes[4] = {JDS_SS_444, JDS_SS_422, JDS_SS_420, JDS_SS_GRAY};
  for (int H = 1; H <= 40; ++H)
    for (int W = 1; W <= 40; ++W)
      for (int m = 0; m < 4; ++m) one_image(H, W, modes[m], (H + W + m) % 3);
  const int th = jds::JI_TH, tw = jds::JI_TW;
  for (int ny = 1; ny <= 3; ++ny)
    for (int nx = 1; nx <= 3; ++nx)
      for (int d = -1; d <= 1; ++d)
        for (int m = 0; m < 4; ++m) one_image(ny * th + d, nx * tw + d, modes[m], (ny + nx + d + m + 4) % 3);
  for (int m = 0; m < 4; ++m) {
    one_image(1, 3 * tw + 2, modes[m], 1);
    one_image(3 * th + 2, 1, modes[m], 1);
    one_image(5, 2 * tw + 3, modes[m], 2);
    one_image(2 * th + 3, 5, modes[m], 2);
  }
  one_batch();
  printf("%ld images, %ld checks, %ld failed\n", g_images, g_checks, g_failed);
  return g_failed ? 1 : 0;
}
