// jds_abi.hip — the C-ABI (include/jds.h): contexts, plans, host-buffer path.
//
// Host side only orchestrates: geometry, quant-table upload, buffer
// management and launches.  All per-pixel / per-coefficient arithmetic runs
// in the HIP kernels of jds_codec.hip; there is no CPU fallback.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <algorithm>
#include <vector>
#include <mutex>
#include <new>
#include <string>
#include <thread>

#include "jds_dct16.hpp"
#include "jds_dct8.hpp"
#include "jds_entropy_mcu_dev.hpp"
#include "jds_huffdec.hpp"
#include "jds_huffopt.hpp"
#include "jds_internal.hpp"
#include "jds_jpeg_inv.hpp"
#include "jds_jpeg_ljt.hpp"
#include "jds_xform_dev.hpp"

#ifdef JDS_INV6
#define JDS_INV6_LIST 1  // the transpose-free variant's tile list (A/B builds: tools/build_variant.py)
#else
#define JDS_INV6_LIST 0
#endif

namespace jds {
hipError_t launch_codec(int mode, bool pf, const Geo& g, int n, const uint8_t* rgb, uint8_t* rgb_out,
                        int16_t* coeffs, const FrameQ* fq, const double* gk, jds_frame_stats* st,
                        double* part, bool want_sse, double* err_y, double* err_rgb, jds_selected_block* sel,
                        int sel_blk, hipStream_t s, hipEvent_t* ev, int phases, int in_div, const GenBufs* gb,
                        const InvFix* fx = nullptr);
int inv_tiles(int mode, int H, int W);
int area_tab_build(int src, int dst, AreaTap* tab);
size_t gen_sub_doubles(const Geo& g);
size_t gen_rec_doubles(const Geo& g);
int gen_px_tiles(const Geo& g);
hipError_t stage_area_gen(const double* in, int H, int W, const AreaTap* ytab, const AreaTap* xtab, double* out,
                          int oh, int ow, hipStream_t s);
hipError_t launch_psnr_ssim_batch(const void* pairs_dev, int items, int H, int W, double c1, double c2,
                                  double* scratch, double* out, int out_stride, unsigned long long* sse,
                                  hipStream_t s, bool rgb, hipStream_t side, hipEvent_t fork, hipEvent_t join);
hipError_t launch_ssim_rgb(const void* pairs_dev, int items, int H, int W, double c1, double c2, double* scratch,
                           double* out, int out_stride, hipStream_t s);
size_t ssim_batch_scratch_doubles(int H, int W, bool rgb, bool planes);
bool ssim_batch_planes(int items);
size_t ssim_rgb_scratch_doubles(int H, int W);
int ssim_batch_max_items();
hipError_t launch_sse_u8(const uint8_t* a, const uint8_t* b, long long n, unsigned long long* out, hipStream_t s);
size_t mag_scratch_bytes(long long nblocks, int max_chunks);
hipError_t launch_mag_f32(const int16_t* coeffs, long long nblocks, unsigned* chunk_sum, int max_chunks,
                          double* out, hipStream_t s);
void combined_taps32(const double* gk, float* out5);
size_t fast_part_words(const Geo& g, int n);
hipError_t launch_fast_fwd(int mode, bool pf, const Geo& g, int n, int nq, const uint8_t* rgb, int16_t* coeffs,
                           const FrameQ* fq, const void* fq32, const double* gk, const float* gk32,
                           jds_frame_stats* st, uint32_t* part, uint32_t* fixbits, uint2* fixlist, unsigned* fixcount,
                           float* dct32,
                           hipStream_t s, bool finish, int par);
int quant_mq_tiles(const Geo& g);
int inv16_tiles(int mode, int H, int W);
constexpr int MAXQ_SHARED = 8;  // jds_fast.hip MAXQ
void fast_fwd_bounds(int mode, bool pf, const double* gk, double* E);
int fwd32_host_plane(int mode, bool pf, const double* gk, const uint8_t* rgb, int H, int W, int plane,
                     int flags, float* out);
void fast_fwd_thresholds(const double* Q, int mode, bool pf, const double* gk, float* rq, float* thr);
int inv_fast_host(int mode, const int16_t* cf, const double* Q, int H, int W, int fuse, int block, double* vout,
                  uint8_t* bout);
size_t fast_q_size();
hipError_t stage_rgb_ycc(const double* in, double* out, long long n, int inverse, hipStream_t s);
hipError_t stage_subsample(const double* in, double* tmp, double* tmp2, double* out, int H, int W, int sy,
                           int prefilter, const double* k, hipStream_t s);
hipError_t stage_resize(const double* in, int h, int w, double* out, int H, int W, int nearest, hipStream_t s);
hipError_t stage_block(const double* in, double* out, long long n, int bs, int op, hipStream_t s);
hipError_t stage_quant(const void* in, const double* q, void* out, long long n, int dequant, int period,
                       hipStream_t s);
int tile_dims16(int mode, int* MY, int* MX);
struct EntTab;
void ent_build_tables(EntTab* t);
size_t ent_tab_size();
int ent_header(const double* q, int mode, int H, int W, uint8_t* o);
long long ent_capacity(const Geo& g);
void ent_sizes(const Geo& g, int n, size_t* sz);
hipError_t launch_entropy(const Geo& g, int n, const int16_t* coeffs, void* const* buf, const uint8_t* hdr_dev,
                          const void* tab_dev, uint8_t* out, long long stride, unsigned long long* lengths,
                          unsigned long long* scan_bits, hipStream_t s);
int ent_restart_interval();
int ent_header_rst(const double* q, int mode, int H, int W, int interval, uint8_t* o);
long long ent_capacity_rst(const Geo& g);
hipError_t launch_entropy_rst(const Geo& g, int n, const int16_t* coeffs, void* const* buf, const uint8_t* hdr_dev,
                              const void* tab_dev, uint8_t* out, long long stride, unsigned long long* lengths,
                              unsigned long long* scan_bits, hipStream_t s);
// the optimised-table route (jds_entropy.hip, jds_huffopt.hip)
long long ent_capacity_opt(const Geo& g, bool rst);
hipError_t launch_entropy_opt(const Geo& g, int n, const int16_t* coeffs, void* const* buf, const uint8_t* hdr_dev,
                              const void* tab_dev, uint8_t* out, long long stride, unsigned long long* lengths,
                              unsigned long long* scan_bits, hipStream_t s);
hipError_t launch_entropy_rst_opt(const Geo& g, int n, const int16_t* coeffs, void* const* buf,
                                  const uint8_t* hdr_dev, const void* tab_dev, uint8_t* out, long long stride,
                                  unsigned long long* lengths, unsigned long long* scan_bits, hipStream_t s);
int ent_std_table(int idx, const uint8_t** bits, const uint8_t** vals);
void opt_table_host(const uint32_t* freq, HoTable* t);
hipError_t launch_opt_tables_selftest(int n, const uint32_t* freq, uint8_t* bits, uint8_t* vals, int32_t* nv,
                                      int32_t* fell, hipStream_t s);
void rst_constants(int* lane_max);
int rst_group_lanes();
size_t rst_work_bytes(int n, const RstGeo& rg);
hipError_t launch_dec_rst(const uint8_t* files, const RstIv* ivs_dev, long long niv, const HuffDecTab* tabs_dev,
                          int16_t* coeffs, uint32_t* status, hipStream_t s, const HdMcu* mcu_dev);
hipError_t launch_dec_rst_plan(const uint8_t* files, long long stride, const unsigned long long* lengths,
                               const uint8_t* hdr_dev, int hl, int n, const RstGeo& rg, void* work,
                               const HuffDecTab* tabs_dev, int16_t* coeffs, uint32_t* status, hipStream_t s);
void dec_constants(int* s, int* g);
long long dec_layout(DecScan* sc, int nscans, int* max_ngrp);
size_t dec_scratch_bytes(long long ngroups, int nscans);
size_t dec_hdr_bytes(int n);
hipError_t launch_dec_hdr(const uint8_t* files, long long stride, const unsigned long long* lengths,
                          const uint8_t* hdr_dev, int hl, int n, void* work, uint32_t* status, hipStream_t s);
hipError_t dec_run(const uint8_t* files, const DecScan* sc, int nscans, long long ngroups, int max_ngrp,
                   const HuffDecTab* tabs_dev, void* scratch, int16_t* coeffs, long long n_coeffs, uint32_t* status,
                   hipStream_t s, unsigned* rounds, int* too_many, const HdMcu* mcu_dev, int16_t* dcs);
hipError_t dec_run_groups(const uint8_t* files, const DecGroup* grp, int ngrp, const HuffDecTab* tabs_dev,
                          int16_t* coeffs, long long n_coeffs, uint32_t* status, hipStream_t s, unsigned* rounds,
                          int* too_many, const HdMcu* mcu_dev, int16_t* dcs);
hipError_t launch_codec16(int mode, bool pf, const Geo& g, int n, const uint8_t* rgb, uint8_t* rgb_out,
                          int16_t* coeffs, const FrameQ* fq, const double* gk, jds_frame_stats* st, double* part,
                          double* planes, bool want_sse, double* err_y, double* err_rgb, hipStream_t s,
                          hipEvent_t* ev, int phases, const Fwd16Fast* ff, const InvFix* fx);
void fast_fwd16_bounds(int mode, bool pf, const double* gk, double* E);
void fast_fwd16_thresholds(const double* Q8, int mode, bool pf, const double* gk, void* out);
size_t fast_q16_size();
int fwd16_host_plane(int mode, bool pf, const double* gk, const uint8_t* rgb, int H, int W, int plane,
                     int flags, float* out);
void jpeg_inv_constants(int* th, int* tw);
bool jpeg_inv_fits(const JInvArgs& a);
hipError_t launch_jpeg_inv(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, hipStream_t s);
void jpeg_inv_host(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb);
hipError_t launch_jpeg_inv_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES],
                                 const int nmap[JI_MODES], const int tiles[JI_MODES], const uint32_t* status,
                                 const int16_t* coeffs, uint8_t* rgb, hipStream_t s);
hipError_t launch_jpeg_ljt(const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, hipStream_t s);
hipError_t launch_jpeg_ljt_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES],
                                 const int nmap[JI_MODES], const int tiles[JI_MODES], const uint32_t* status,
                                 const int16_t* coeffs, uint8_t* rgb, hipStream_t s);
}

// skimage: C1 = (K1 * R) ** 2, C2 = (K2 * R) ** 2 with R = data_range = 255
static const double SSIM_C1 = (0.01 * 255) * (0.01 * 255);
static const double SSIM_C2 = (0.03 * 255) * (0.03 * 255);

using namespace jds;

static thread_local char g_err[512] = "";

static int fail(int code, const char* fmt, ...) {
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(g_err, sizeof g_err, fmt, ap);
  va_end(ap);
  return code;
}

#define HIP_TRY(expr)                                                                       \
  do {                                                                                      \
    hipError_t e_ = (expr);                                                                 \
    if (e_ != hipSuccess)                                                                   \
      return fail(e_ == hipErrorOutOfMemory ? JDS_ENOMEM : JDS_EHIP, "%s: %s (%s:%d)", #expr, \
                  hipGetErrorString(e_), __FILE__, __LINE__);                               \
  } while (0)

struct DevBuf {
  void* p = nullptr;
  size_t n = 0;
  hipError_t ensure(size_t bytes) {
    if (bytes <= n) return hipSuccess;
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
    hipError_t e = hipMalloc(&p, bytes ? bytes : 1);
    if (e == hipSuccess) n = bytes;
    return e;
  }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    n = 0;
  }
};

struct jds_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipEvent_t ev[3] = {nullptr, nullptr, nullptr};
  // host path: the device -> host copies run on a stream of their own beside
  // the statistics kernels (SSIM, float32 magnitude bits) of the same call
  hipStream_t xfer = nullptr;
  hipEvent_t xfer_ev = nullptr;
  // SSIM: the R, G, B rows kernels run on a stream of its own beside the luma
  // planes, chains and band (jds_ssim_band.hip); ss_pairs: the batch's image
  // pointers (pinned host staging, device copy)
  hipStream_t ss_side = nullptr;
  hipEvent_t ss_fork = nullptr, ss_join = nullptr;
  void* ss_pairs_host = nullptr;
  size_t ss_pairs_cap = 0;
  // host-path scratch
  DevBuf rgb, out, coeffs, stats, part, fq, gk, erry, errrgb, sel;
  DevBuf ss_planes, ss_out, img_a, img_b;  // ss_planes: k_ss_* scratch
  DevBuf ss_rgb, ss_pairs;                 // k_ss_rows / k_ss_rgbsum scratch, device pair array
  DevBuf st[5];  // per-stage API staging
  DevBuf chunks;
  DevBuf planes;  // 16x16 path: reconstructed chroma planes
  DevBuf ent[8], ent_hdr, ent_tab, ent_cf, ent_out, ent_meta;  // entropy coder (jds_encode_jfif)
  DevBuf dec_file, dec_tab, dec_scr, dec_st;  // entropy decoder (jds_decode_jfif): file, tables, scratch, status
  DevBuf dec_iv;                              // its restart interval table
  DevBuf dec_mcu;                             // interleaved scans (jds_decode_jpeg): MCU descriptor, DC staging array
  // jds_jpeg_batch_to_rgb: everything a batch uploads (file bytes, table sets, MCU and inverse records, tile maps,
  // interval lists, initial status words) is gathered in one pinned host buffer and copied once to bat
  DevBuf bat;
  DevBuf mcu_up, mcu_scr;  // interleaved-scan writer (jds_jpeg_transcode): its uploads (records, segment table, prefixes), scratch
  void* bat_host = nullptr;
  size_t bat_host_cap = 0;
  // jds_ctx_profile: launch marks of the batch calls on this context
  KMarks marks;
  bool prof_on = false;
  DevBuf gen_tab, gen_sub, gen_rec;  // general-geometry path (jds_gen.hip)
  size_t ss_budget = 0;  // SSIM scratch budget per launch group (0: SSIM_SCRATCH; jds_ctx_set_ssim_scratch)
};

// batches from this size take the R, G, B rows kernel (jds_ssim_band.hip)
constexpr int SSIM_ROWS_MIN = 32;
// SSIM scratch (luma planes, chain checkpoints, maps) per launch group
constexpr size_t SSIM_SCRATCH = (size_t)16 << 30;

// SSIM of `items` image pairs (K4, jds_ssim_band.hip) on the context's stream:
// out[i * out_stride + 0..4] = SSIM R, G, B, Y, MSE of Y (device doubles);
// sse[i] (nullable, zeroed here) = the pair's integer RGB squared-error sum.
// Batches beyond the kernel's per-launch limit run as consecutive launches.
static int run_ssim_batch(jds_ctx* c, int items, const uint8_t* const* a, const uint8_t* const* b, int H, int W,
                          double* out, int out_stride, unsigned long long* sse) {
  // R, G, B: batches of SSIM_ROWS_MIN items or more take the rows kernel (one
  // lane per map row, every item in one launch: its grid fills the chip only
  // with many items); smaller ones the band kernel beside each luma group
  const bool rows = items >= SSIM_ROWS_MIN && (unsigned long long)H * W * 3ull < (1ull << 31);  // (32-bit staging)
  const int per = ssim_batch_max_items();
  // luma (and small batches' RGB) scratch: as many items per launch as the
  // budget holds (1080p: ~27 MB per item; launches under 8 pairs keep fp64
  // luma planes, ~60 MB, ~110 MB with RGB maps) -- the luma chains, like the
  // rows, are latency-bound per lane and need many items in flight.  A
  // launch's layout (planes or not) follows its own size, so the group size
  // is settled first and the scratch sized for the groups that actually run:
  // the full groups and the remainder.
  const size_t budget = c->ss_budget ? c->ss_budget : SSIM_SCRATCH;
  auto bytes_of = [&](int k) {  // scratch of one launch of k pairs
    return ssim_batch_scratch_doubles(H, W, !rows, ssim_batch_planes(k)) * sizeof(double) * (size_t)k;
  };
  int group = std::min(per, items);
  if (bytes_of(group) > budget) {
    const size_t each_np = ssim_batch_scratch_doubles(H, W, !rows, false) * sizeof(double);
    group = (int)std::max<size_t>(1, std::min<size_t>((size_t)group, budget / each_np));
    if (ssim_batch_planes(group) && bytes_of(group) > budget) {  // the planes layout: larger per item
      const size_t each_p = ssim_batch_scratch_doubles(H, W, !rows, true) * sizeof(double);
      group = (int)std::max<size_t>(1, std::min<size_t>((size_t)group, budget / each_p));
    }
  }
  size_t need = bytes_of(group);
  const int last = items % group;
  if (last) need = std::max(need, bytes_of(last));
  HIP_TRY(c->ss_planes.ensure(need));
  if (!c->ss_side) {
    HIP_TRY(hipStreamCreateWithFlags(&c->ss_side, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->ss_fork, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ss_join, hipEventDisableTiming));
  }
  // the pair array: pinned staging (reused only after the previous call's
  // final synchronisation) -> device, on the context's stream
  const size_t pbytes = sizeof(const void*) * 2 * (size_t)items;
  if (c->ss_pairs_cap < pbytes) {
    if (c->ss_pairs_host) HIP_TRY(hipHostFree(c->ss_pairs_host));
    c->ss_pairs_host = nullptr;
    c->ss_pairs_cap = 0;
    HIP_TRY(hipHostMalloc(&c->ss_pairs_host, pbytes, hipHostMallocDefault));
    c->ss_pairs_cap = pbytes;
  }
  const void** ph = (const void**)c->ss_pairs_host;
  for (int i = 0; i < items; ++i) {
    ph[2 * i] = a[i];
    ph[2 * i + 1] = b[i];
  }
  HIP_TRY(c->ss_pairs.ensure(pbytes));
  HIP_TRY(hipMemcpyAsync(c->ss_pairs.p, ph, pbytes, hipMemcpyHostToDevice, c->stream));
  auto pairs_at = [&](int i0) { return (const void*)((const char*)c->ss_pairs.p + sizeof(const void*) * 2 * (size_t)i0); };
  if (sse) HIP_TRY(hipMemsetAsync(sse, 0, sizeof(unsigned long long) * items, c->stream));
  if (rows) {
    // as many items per launch as ~4 GB of scratch holds (1080p: ~4 MB per item)
    const size_t each_rgb = ssim_rgb_scratch_doubles(H, W) * sizeof(double);
    const int group_rgb = (int)std::min<size_t>((size_t)items, std::max<size_t>(1, ((size_t)4 << 30) / each_rgb));
    HIP_TRY(c->ss_rgb.ensure(each_rgb * group_rgb));
    // on the side stream (after the copy and the stream's earlier work), beside
    // the luma groups on the context's stream; joined at the end
    HIP_TRY(hipEventRecord(c->ss_fork, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->ss_side, c->ss_fork, 0));
    for (int i0 = 0; i0 < items; i0 += group_rgb) {
      const int k = std::min(group_rgb, items - i0);
#ifdef JDS_SSIM_PROBE_NORGB  // tools: timing probes only (wrong values)
      continue;
#endif
      HIP_TRY(launch_ssim_rgb(pairs_at(i0), k, H, W, SSIM_C1, SSIM_C2, (double*)c->ss_rgb.p,
                              out + (size_t)i0 * out_stride, out_stride, c->ss_side));
    }
    HIP_TRY(hipEventRecord(c->ss_join, c->ss_side));
  }
  for (int i0 = 0; i0 < items; i0 += group) {
    const int k = std::min(group, items - i0);
#ifdef JDS_SSIM_PROBE_NOLUMA  // tools: timing probes only (wrong values)
    if (rows) continue;
#endif
    HIP_TRY(launch_psnr_ssim_batch(pairs_at(i0), k, H, W, SSIM_C1, SSIM_C2, (double*)c->ss_planes.p,
                                   out + (size_t)i0 * out_stride, out_stride, sse ? sse + i0 : nullptr, c->stream,
                                   !rows, c->ss_side, c->ss_fork, c->ss_join));
  }
  if (rows) HIP_TRY(hipStreamWaitEvent(c->stream, c->ss_join, 0));
  return JDS_OK;
}

// one pair; returns the device pointer of 5 result doubles in dres
static int run_ssim(jds_ctx* c, const uint8_t* a, const uint8_t* b, int H, int W, double* dres) {
  return run_ssim_batch(c, 1, &a, &b, H, W, dres, 5, nullptr);
}

struct jds_plan {
  jds_ctx* ctx = nullptr;
  int n = 0, mode = 0;
  int nq = 1;      // tables per frame (sweep plan): items = frames * nq, item = frame * nq + q
  DevBuf dct32;    // sweep plans: fp32 coefficients of every frame (shared front end)
  bool pf = false;
  Geo g{};
  DevBuf fq, gk, part;
  // fast path: fp32 tables, fix-up lists and counters
  DevBuf fq32, gk32, fixbits, fixlist, counters, part32;  // per-item fix-up bitmaps and lists; per-tile statistics
  DevBuf invfix;  // certified fast inverse: run and per-item counters (InvFix, jds_inv_fast.hip)
  DevBuf invlist;  // k_inv_fast6 (4:2:0, -DJDS_INV6 builds): the tiles a run hands to the exact kernel (InvFix::list)
  unsigned inv_runs = 0;  // fast-inverse runs so far: picks the list counter (InvFix::parity)
  bool last_inv_fast = false;  // the last run's inverse was the certified fast one
  // Where the certified fast inverse pays (measured, 1 MI355X): 4:2:x plans
  // whose tables are not coarse.  Coarse tables (DC quantiser > 60: quality
  // below ~14 on the standard table) put most tiles on the exact path
  // (reconstructions land on integers), where k_inv2 beats k_inv_fast's
  // in-kernel fallback (4K 4:2:0: Q10 373 vs 396 us; Q20 376 vs 347).  At
  // 4:4:4 the wave-local k_inv_fast444 is faster at every quality (512x512 x
  // 256: 167.5 vs k_inv2's 331.8 us).
  bool inv_fast_ok = true;
  // some item's table is not coarse: mixed plans (quality sweeps) run the
  // certified inverse too, their coarse items seeded into its per-item exact
  // mode (InvFix), so every item takes the faster kernel for its table
  bool inv_fast_any = true;
  bool last_fwd16_fast = false;  // 16x16: the last forward was the certified fp32 one
  unsigned fwd16_runs = 0;       // 16x16 certified forward runs so far: picks the list counter
  unsigned fwd8_runs = 0;        // 8x8 single-quality certified forward runs: picks the counter bank
  int last_fwd8_bank = -1;       // bank of the last such run (jds_plan_fix_counts), -1: none
  InvFix inv_fix() const {
    return {(unsigned*)invfix.p, (unsigned*)invfix.p + 16, 0, (int)(inv_runs & 1u), (int)(inv_runs % 3u),
            (int)(inv_runs % 16u == 15u), (uint2*)invlist.p};
  }
  DevBuf planes;  // 16x16 path: reconstructed chroma planes (n x 2 x hc x wc f64)
  double* qt = nullptr;  // host copy of the per-frame 8x8 tables (entropy headers)
  DevBuf ent[8], ent_hdr, ent_tab;  // entropy coder scratch, allocated by the first jds_plan_entropy
  DevBuf dec_tab, dec_scr, dec_info;  // entropy decoder (jds_plan_entropy_decode): tables, scratch, scan ranges
  unsigned dec_rounds = 0;            // propagation rounds of the last decode
  DevBuf rst_hdr, rst_work;           // jds_plan_entropy_decode_rst: restart header templates, interval table and marker list
  int rst_hdr_interval = 0;           // the interval rst_hdr was built for
  DevBuf gen_tab, gen_sub, gen_rec;  // general-geometry path (jds_gen.hip)
  GenBufs gen() const { return {(const AreaTap*)gen_tab.p, (double*)gen_sub.p, (double*)gen_rec.p}; }
  // jds_plan_profile: the launch marks of profiled runs (event pool + names)
  bool prof_on = false;
  KMarks marks;
};

namespace jds {
thread_local KMarks* t_kmarks = nullptr;

void kmark(hipStream_t s, const char* fmt, ...) {
  KMarks* m = t_kmarks;
  if (!m) return;
  if (m->n >= m->cap) {  // reported by jds_plan_profile_read (the totals would be short)
    m->dropped++;
    return;
  }
  if (hipEventRecord(m->ev[m->n], s) != hipSuccess) return;
  va_list ap;
  va_start(ap, fmt);
  vsnprintf(m->name[m->n], sizeof m->name[0], fmt, ap);
  va_end(ap);
  m->n++;
}
}  // namespace jds

// Marks the runs of a profiled plan on this thread (jds_plan_run's scope).
struct MarkScope {
  explicit MarkScope(jds_plan* p, hipStream_t s) {
    if (!p->prof_on) return;
    t_kmarks = &p->marks;
    kmark(s, "(between runs)");
  }
  ~MarkScope() { t_kmarks = nullptr; }
};

// The same for a profiled context (jds_jpeg_batch_to_rgb's scope).
struct CtxMarkScope {
  explicit CtxMarkScope(jds_ctx* c, hipStream_t s) {
    if (!c->prof_on) return;
    t_kmarks = &c->marks;
    kmark(s, "(between calls)");
  }
  ~CtxMarkScope() { t_kmarks = nullptr; }
};

static void marks_release(KMarks& m) {
  for (int i = 0; i < m.cap; ++i) (void)hipEventDestroy(m.ev[i]);
  free(m.ev);
  free(m.name);
  m = KMarks{};
}

// ------------------------------------------------------------- geometry --

static int make_geo(const jds_params* p, int64_t H, int64_t W, Geo* g, int* mode_out, bool* pf_out) {
  if (!p || !g) return fail(JDS_EINVAL, "null argument");
  // 8: the reference's path.  16: the configs[4] stretch (jds_b16.hip; table
  // np.kron(Q8, ones((2,2)))).  Anything else fails the way the reference's
  // quantizer does (engines/quantizer.py:24).
  if (p->block_size != 8 && p->block_size != 16)
    return fail(JDS_ENOTSUP, "operands could not be broadcast together with shapes (%d,%d) (8,8) ",
                p->block_size, p->block_size);
  const int B = p->block_size;
  if (p->subsampling < JDS_SS_444 || p->subsampling > JDS_SS_420)
    return fail(JDS_EINVAL, "Unknown subsampling mode: %d", p->subsampling);
  if (H < 1 || W < 1 || H > 65536 || W > 65536 || H * W > (int64_t)1 << 28)
    return fail(JDS_EINVAL, "unsupported image size %lldx%lld", (long long)H, (long long)W);
  const int mode = p->subsampling;
  const int sy = mode == JDS_SS_420 ? 2 : 1, sx = mode == JDS_SS_444 ? 1 : 2;
  // cv2.resize(c, (W // 2, H // sy), INTER_AREA) (engines/color_space.py:42-49)
  // asserts a non-empty destination
  if (H / sy < 1 || W / sx < 1)
    return fail(JDS_EINVAL,
                "OpenCV(4.8.0) resize.cpp: error: (-215:Assertion failed) !dsize.empty() in function 'resize' "
                "(image %lldx%lld, %s)",
                (long long)H, (long long)W, mode == JDS_SS_420 ? "4:2:0" : "4:2:2");
  // odd H (4:2:0) or odd W (4:2:x): cv2's fractional INTER_AREA and non-2x
  // INTER_LINEAR -> the general-geometry kernels (jds_gen.hip)
  const bool gen = (sy == 2 && (H % 2)) || (sx == 2 && (W % 2));
  if (gen && B == 16)
    return fail(JDS_ENOTSUP, "16x16 blocks with an odd %s image size (%lldx%lld) are not supported",
                mode == JDS_SS_420 ? "4:2:0" : "4:2:2", (long long)H, (long long)W);
  Geo& G = *g;
  memset(&G, 0, sizeof G);
  G.H = (int)H;
  G.W = (int)W;
  G.hc = (int)(H / sy);
  G.wc = (int)(W / sx);
  G.bs = B;
  G.gen = gen ? 1 : 0;
  if (gen) area_fast_scales((int)H, (int)(H / sy), (int)W, (int)(W / sx), &G.afy, &G.afx);
  G.nby = (int)((H + B - 1) / B);
  G.nbx = (int)((W + B - 1) / B);
  G.ncy = (G.hc + B - 1) / B;
  G.ncx = (G.wc + B - 1) / B;
  int MY, MX;
  if (B == 16) (void)tile_dims16(mode, &MY, &MX);
  else switch (mode) {
    case JDS_SS_420: MY = Cfg<M420>::MY; MX = Cfg<M420>::MX; break;
    case JDS_SS_422: MY = Cfg<M422>::MY; MX = Cfg<M422>::MX; break;
    default: MY = Cfg<M444>::MY; MX = Cfg<M444>::MX; break;
  }
  G.nmy = mode == JDS_SS_444 ? G.nby : G.ncy;
  G.nmx = mode == JDS_SS_444 ? G.nbx : G.ncx;
  G.tiles_y = (G.nmy + MY - 1) / MY;
  G.tiles_x = (G.nmx + MX - 1) / MX;
  G.ty_off = G.tiles_y * MY - G.nmy;
  G.tx_off = G.tiles_x * MX - G.nmx;
  const long long yb = (long long)G.nby * G.nbx, cb = (long long)G.ncy * G.ncx;
  G.cpf = (long long)B * B * (yb + 2 * cb);
  G.off_cb = (long long)B * B * yb;
  G.off_cr = (long long)B * B * (yb + cb);
  // cv2.resize: inv_scale = dst/src, scale = 1/inv_scale
  G.up_sy = 1.0 / ((double)H / (double)G.hc);
  G.up_sx = 1.0 / ((double)W / (double)G.wc);
  if (mode_out) *mode_out = mode;
  if (pf_out) *pf_out = mode != JDS_SS_444 && p->prefilter != 0;
  return JDS_OK;
}

static void fill_geometry(const Geo& G, int mode, jds_geometry* o) {
  o->H = G.H;
  o->W = G.W;
  o->chroma_h = G.hc;
  o->chroma_w = G.wc;
  o->y_blocks_y = G.nby;
  o->y_blocks_x = G.nbx;
  o->c_blocks_y = G.ncy;
  o->c_blocks_x = G.ncx;
  o->coeffs_per_frame = G.cpf;
  o->cb_offset = G.off_cb;
  o->cr_offset = G.off_cr;
  o->tiles = G.tiles_y * G.tiles_x;
  if (G.bs == 16) {
    int my, mx;
    o->threads_fwd = tile_dims16(mode, &my, &mx);
    o->threads_inv = 256;
  } else {
    o->threads_fwd = mode == JDS_SS_420 ? Cfg<M420>::TF : mode == JDS_SS_422 ? Cfg<M422>::TF : Cfg<M444>::TF;
    o->threads_inv = Cfg<M420>::TI;
  }
  o->reserved = 0;
}

static void make_fq(const jds_params* p, FrameQ* q) {
  q->qmax = 0.0;
  q->pad_ = 0.0;
  for (int i = 0; i < 64; ++i) {
    q->q[i] = p->qtable[i];
    q->q16[i] = 16.0 * p->qtable[i];  // exact
    q->qmax = q->qmax > p->qtable[i] ? q->qmax : p->qtable[i];
  }
}

// scale_quant_matrix (engines/quantizer.py:7-19) yields integers in [1, 255]
// (floor, then clip); the kernels rely on it (integer dequantisation).
static int check_tables(const jds_params* p) {
  for (int i = 0; i < 64; ++i) {
    if (!(p->qtable[i] >= 1.0 && p->qtable[i] <= 255.0))
      return fail(JDS_EINVAL, "qtable[%d] = %g outside [1, 255]", i, p->qtable[i]);
    if (p->qtable[i] != floor(p->qtable[i]))
      return fail(JDS_EINVAL, "qtable[%d] = %g is not an integer", i, p->qtable[i]);
  }
  return JDS_OK;
}

// Area tables (y then x) and plane scratch of the general-geometry path for
// n items of n_frames frames.
static int gen_prepare(const Geo& g, int n_frames, int n, DevBuf& tab, DevBuf& sub, DevBuf& rec, hipStream_t s) {
  const size_t nt = (size_t)g.hc + g.wc;
  AreaTap* h = (AreaTap*)malloc(sizeof(AreaTap) * nt);
  if (!h) return fail(JDS_ENOMEM, "host allocation failed");
  if (area_tab_build(g.H, g.hc, h) < 0 || area_tab_build(g.W, g.wc, h + g.hc) < 0) {
    free(h);
    return fail(JDS_EINVAL, "INTER_AREA table with more than 4 taps per sample (%dx%d)", g.H, g.W);
  }
  hipError_t e = tab.ensure(sizeof(AreaTap) * nt);
  if (e == hipSuccess) e = hipMemcpyAsync(tab.p, h, sizeof(AreaTap) * nt, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // h is freed below
  free(h);
  HIP_TRY(e);
  HIP_TRY(sub.ensure(sizeof(double) * gen_sub_doubles(g) * (size_t)n_frames));
  HIP_TRY(rec.ensure(sizeof(double) * gen_rec_doubles(g) * (size_t)n));
  return JDS_OK;
}

// ------------------------------------------------------------------ ABI --

// fn(i) for i in [0, n) on up to BATCH_THREADS host threads (files are
// independent: a 1080p file's parse walks its 850 KB of scan data for markers,
// and its gather copies them).
constexpr int BATCH_THREADS = 8;
template <class F>
static void batch_parallel(int n, F fn) {
  const int nt = n < 4 ? 1 : (n / 2 < BATCH_THREADS ? n / 2 : BATCH_THREADS);
  if (nt <= 1) {
    for (int i = 0; i < n; ++i) fn(i);
    return;
  }
  std::vector<std::thread> th;
  th.reserve((size_t)nt);
  for (int t = 1; t < nt; ++t) {
    auto share = [=] {
      for (int i = t; i < n; i += nt) fn(i);
    };
    try {
      th.emplace_back(share);
    } catch (...) {  // no thread to be had: this one does the share
      share();
    }
  }
  for (int i = 0; i < n; i += nt) fn(i);
  for (std::thread& t : th) t.join();
}

extern "C" {

int jds_abi_version(void) { return JDS_ABI_VERSION; }

const char* jds_last_error(void) { return g_err; }

int jds_device_count(int* n) {
  if (!n) return fail(JDS_EINVAL, "null argument");
  int c = 0;
  hipError_t e = hipGetDeviceCount(&c);
  if (e != hipSuccess) {
    *n = 0;
    return fail(JDS_EHIP, "hipGetDeviceCount: %s", hipGetErrorString(e));
  }
  *n = c;
  return JDS_OK;
}

void* jds_ctx_stream(jds_ctx* c) { return c ? (void*)c->stream : nullptr; }

int jds_ctx_set_ssim_scratch(jds_ctx* c, int64_t bytes) {
  if (!c) return fail(JDS_EINVAL, "null argument");
  c->ss_budget = bytes > 0 ? (size_t)bytes : 0;
  return JDS_OK;
}

int jds_geometry_of(const jds_params* p, int64_t H, int64_t W, jds_geometry* out) {
  Geo g;
  int mode;
  int rc = make_geo(p, H, W, &g, &mode, nullptr);
  if (rc) return rc;
  if (!out) return fail(JDS_EINVAL, "null argument");
  fill_geometry(g, mode, out);
  return JDS_OK;
}

int jds_ctx_create(int device, jds_ctx** out) {
  if (!out) return fail(JDS_EINVAL, "null argument");
  int n = 0;
  HIP_TRY(hipGetDeviceCount(&n));
  if (device < 0 || device >= n) return fail(JDS_EINVAL, "device %d out of range (%d devices)", device, n);
  HIP_TRY(hipSetDevice(device));
  jds_ctx* c = new (std::nothrow) jds_ctx();
  if (!c) return fail(JDS_ENOMEM, "host allocation failed");
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return fail(JDS_EHIP, "hipStreamCreate: %s", hipGetErrorString(e));
  }
  for (int i = 0; i < 3; ++i) {
    if ((e = hipEventCreate(&c->ev[i])) != hipSuccess) {
      jds_ctx_destroy(c);
      return fail(JDS_EHIP, "hipEventCreate: %s", hipGetErrorString(e));
    }
  }
  *out = c;
  return JDS_OK;
}

void jds_ctx_destroy(jds_ctx* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  (void)hipStreamSynchronize(c->stream);
  if (c->xfer) {
    (void)hipStreamSynchronize(c->xfer);
    (void)hipStreamDestroy(c->xfer);
  }
  if (c->xfer_ev) (void)hipEventDestroy(c->xfer_ev);
  if (c->ss_side) {
    (void)hipStreamSynchronize(c->ss_side);
    (void)hipStreamDestroy(c->ss_side);
  }
  if (c->ss_fork) (void)hipEventDestroy(c->ss_fork);
  if (c->ss_join) (void)hipEventDestroy(c->ss_join);
  if (c->ss_pairs_host) (void)hipHostFree(c->ss_pairs_host);
  c->ss_rgb.release();
  c->ss_pairs.release();
  DevBuf* bufs[] = {&c->rgb,     &c->out,    &c->coeffs,    &c->stats,  &c->part,  &c->fq,   &c->gk,  &c->erry,
                    &c->errrgb,  &c->sel,    &c->ss_planes, &c->ss_out, &c->img_a, &c->img_b};
  for (DevBuf* b : bufs) b->release();
  for (DevBuf& b : c->st) b.release();
  c->chunks.release();
  c->planes.release();
  for (DevBuf& b : c->ent) b.release();
  c->ent_hdr.release();
  c->ent_tab.release();
  c->ent_cf.release();
  c->ent_out.release();
  c->ent_meta.release();
  c->dec_file.release();
  c->dec_tab.release();
  c->dec_scr.release();
  c->dec_st.release();
  c->dec_iv.release();
  c->dec_mcu.release();
  c->bat.release();
  c->mcu_up.release();
  c->mcu_scr.release();
  if (c->bat_host) (void)hipHostFree(c->bat_host);
  marks_release(c->marks);
  c->gen_tab.release();
  c->gen_sub.release();
  c->gen_rec.release();
  for (hipEvent_t e : c->ev)
    if (e) (void)hipEventDestroy(e);
  (void)hipStreamDestroy(c->stream);
  delete c;
}

int jds_plan_create(jds_ctx* ctx, const jds_params* params, int n, int64_t H, int64_t W, jds_plan** out) {
  return jds_plan_create_q(ctx, params, n, 1, H, W, out);
}

int jds_plan_create_q(jds_ctx* ctx, const jds_params* params, int n_frames, int n_q, int64_t H, int64_t W,
                      jds_plan** out) {
  if (!ctx || !params || !out || n_frames < 1 || n_q < 1 || (long long)n_frames * n_q > (1 << 24))
    return fail(JDS_EINVAL, "bad argument");
  if (n_q > 1 && params[0].block_size != 8)
    return fail(JDS_ENOTSUP, "quality sweep plans (n_q > 1) need 8x8 blocks");
  if (n_q > MAXQ_SHARED) return fail(JDS_ENOTSUP, "at most %d tables per frame in a sweep plan", MAXQ_SHARED);
  const int n = n_frames * n_q;
  Geo g;
  int mode;
  bool pf;
  int rc = make_geo(params, H, W, &g, &mode, &pf);
  if (rc) return rc;
  FrameQ* hq = (FrameQ*)malloc(sizeof(FrameQ) * (size_t)n);
  if (!hq) return fail(JDS_ENOMEM, "host allocation failed");
  for (int i = 0; i < n; ++i) {
    if (params[i].subsampling != params[0].subsampling || params[i].block_size != params[0].block_size ||
        (params[i].prefilter != 0) != (params[0].prefilter != 0) ||
        (pf && memcmp(params[i].gauss, params[0].gauss, sizeof params[0].gauss) != 0)) {
      free(hq);
      return fail(JDS_EINVAL, "all frames of a plan must share subsampling / prefilter (taps) / block size");
    }
    if ((rc = check_tables(params + i))) {
      free(hq);
      return rc;
    }
    make_fq(params + i, hq + i);
  }
  HIP_TRY(hipSetDevice(ctx->device));
  jds_plan* p = new (std::nothrow) jds_plan();
  if (!p) {
    free(hq);
    return fail(JDS_ENOMEM, "host allocation failed");
  }
  p->ctx = ctx;
  p->n = n;
  p->nq = n_q;
  p->qt = (double*)malloc(sizeof(double) * 64 * (size_t)n);
  if (!p->qt) {
    free(hq);
    delete p;
    return fail(JDS_ENOMEM, "host allocation failed");
  }
  for (int i = 0; i < n; ++i) memcpy(p->qt + 64 * i, params[i].qtable, 64 * sizeof(double));
  // coarse tables (DC quantiser > 60, quality below ~14) put most tiles of a
  // frame on the certified inverse's fallback (reconstructions land on
  // integers: clipped luma, all-zero chroma), where k_inv2 is faster (16 x 4K
  // 4:2:0 Q10: 358 vs 410 us; an exact-value certificate variant, 425 us, did
  // not pay either -- DESIGN.md): such plans run k_inv2 unless JDS_RUN_INV_FAST
  p->inv_fast_ok = true;
  p->inv_fast_any = mode == JDS_SS_444;
  if (mode != JDS_SS_444)
    for (int i = 0; i < n; ++i) {
      p->inv_fast_ok = p->inv_fast_ok && params[i].qtable[0] <= 60.0;
      p->inv_fast_any = p->inv_fast_any || params[i].qtable[0] <= 60.0;
    }
  p->mode = mode;
  p->pf = pf;
  p->g = g;
  hipError_t e;
  if ((e = p->fq.ensure(sizeof(FrameQ) * n)) != hipSuccess || (e = p->gk.ensure(3 * sizeof(double))) != hipSuccess ||
      (e = p->part.ensure(sizeof(double) * (size_t)n *
                          (size_t)std::max(std::max(g.tiles_y * g.tiles_x, g.gen ? gen_px_tiles(g) : 0),
                                           g.bs == 16 ? inv16_tiles(mode, (int)H, (int)W) : 0))) !=
          hipSuccess ||
      (e = hipMemcpy(p->fq.p, hq, sizeof(FrameQ) * n, hipMemcpyHostToDevice)) != hipSuccess ||
      (e = hipMemcpy(p->gk.p, params[0].gauss, 3 * sizeof(double), hipMemcpyHostToDevice)) != hipSuccess) {
    free(hq);
    p->fq.release();
    p->gk.release();
    p->part.release();
    delete p;
    return fail(e == hipErrorOutOfMemory ? JDS_ENOMEM : JDS_EHIP, "plan upload: %s", hipGetErrorString(e));
  }
  free(hq);
  if (g.gen) {
    // general geometry: exact fp64 kernels over HBM planes (jds_gen.hip)
    if ((rc = gen_prepare(g, n_frames, n, p->gen_tab, p->gen_sub, p->gen_rec, ctx->stream))) {
      jds_plan_destroy(p);
      return rc;
    }
  } else if (g.bs == 16) {
    // 16x16 stretch path (jds_b16.hip, jds_fast16.hip): chroma planes scratch
    // (4:4:4 inverse), the certified forward's fp32 tables, fix-up list, counters
    const size_t fqs = fast_q16_size();
    char* h16 = (char*)malloc(fqs * (size_t)n);
    if (!h16) {
      jds_plan_destroy(p);
      return fail(JDS_ENOMEM, "host allocation failed");
    }
    for (int i = 0; i < n; ++i) fast_fwd16_thresholds(params[i].qtable, mode, pf, params[i].gauss, h16 + fqs * i);
    float gk32[5];  // taps + the combined taps of k_fwd16f's fast staging
    combined_taps32(params[0].gauss, gk32);
    const size_t nblk = (size_t)n * (size_t)(g.cpf / 256);
    if ((e = p->planes.ensure(mode == JDS_SS_444 ? sizeof(double) * 2 * (size_t)n * g.hc * g.wc : 8)) !=
            hipSuccess ||
        (e = p->fq32.ensure(fqs * n)) != hipSuccess || (e = p->gk32.ensure(sizeof gk32)) != hipSuccess ||
        (e = p->fixlist.ensure(8 * nblk)) != hipSuccess || (e = p->counters.ensure(64)) != hipSuccess ||
        (e = p->invfix.ensure(64 + 12 * (size_t)n)) != hipSuccess ||
        (e = hipMemset(p->invfix.p, 0, 64 + 12 * (size_t)n)) != hipSuccess ||
        (e = p->part32.ensure(sizeof(uint32_t) * 52 * (size_t)n * g.tiles_y * g.tiles_x)) != hipSuccess ||
        (e = hipMemcpy(p->fq32.p, h16, fqs * n, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(p->gk32.p, gk32, sizeof gk32, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemset(p->counters.p, 0, 64)) != hipSuccess) {
      free(h16);
      jds_plan_destroy(p);
      return fail(e == hipErrorOutOfMemory ? JDS_ENOMEM : JDS_EHIP, "plan upload: %s", hipGetErrorString(e));
    }
    free(h16);
  } else {
    const size_t fqs = fast_q_size();
    char* h32 = (char*)malloc(fqs * (size_t)n);
    if (!h32) {
      jds_plan_destroy(p);
      return fail(JDS_ENOMEM, "host allocation failed");
    }
    for (int i = 0; i < n; ++i) {
      float* f = (float*)(h32 + fqs * i);
      fast_fwd_thresholds(params[i].qtable, mode, pf, params[i].gauss, f, f + 64);
    }
    // taps and k_fwd32i's combined taps (Gaussian then 2-sample area: k0, k0+k1, k1+k2, k2)
    const double* gs = params[0].gauss;
    float gk32[5];
    combined_taps32(gs, gk32);
    const size_t nblk = (size_t)n * (size_t)(g.cpf / 64);
    const size_t ptiles = (size_t)(n_q > 1 ? quant_mq_tiles(g) : g.tiles_y * g.tiles_x);
    if ((e = p->fq32.ensure(fqs * n)) != hipSuccess || (e = p->gk32.ensure(sizeof gk32)) != hipSuccess ||
        (e = p->fixbits.ensure(4 * (size_t)n * (size_t)fix_wpi(g))) != hipSuccess ||
        (e = p->fixlist.ensure(8 * nblk)) != hipSuccess ||
        (e = p->counters.ensure(8 * (size_t)n + 64)) != hipSuccess ||
        (e = p->part32.ensure(sizeof(uint32_t) * (n_q > 1 ? 52 * (size_t)n * ptiles
                                                          : std::max((size_t)52 * n * ptiles, fast_part_words(g, n))))) !=
            hipSuccess ||
        (e = hipMemset(p->part32.p, 0, p->part32.n)) != hipSuccess ||
        (e = p->invfix.ensure(64 + 12 * (size_t)n)) != hipSuccess ||
        (e = hipMemset(p->invfix.p, 0, 64 + 12 * (size_t)n)) != hipSuccess ||
        (JDS_INV6_LIST && mode == JDS_SS_420 && (e = p->invlist.ensure(8 * (size_t)n * inv_tiles(mode, (int)H, (int)W))) != hipSuccess) ||
        (n_q > 1 && (e = p->dct32.ensure(sizeof(float) * (size_t)n_frames * g.cpf)) != hipSuccess) ||
        (e = hipMemcpy(p->fq32.p, h32, fqs * n, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(p->gk32.p, gk32, sizeof gk32, hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemset(p->counters.p, 0, 8 * (size_t)n + 64)) != hipSuccess ||
        (e = hipMemset(p->fixbits.p, 0, 4 * (size_t)n * (size_t)fix_wpi(g))) != hipSuccess) {
      // the fix-up bitmaps start clean once; k_fix_compact clears the words it consumes
      free(h32);
      jds_plan_destroy(p);
      return fail(e == hipErrorOutOfMemory ? JDS_ENOMEM : JDS_EHIP, "plan upload: %s", hipGetErrorString(e));
    }
    free(h32);
    if (p->inv_fast_any && !p->inv_fast_ok) {
      // mixed tables: the coarse items start in the certified inverse's exact
      // mode (every rotation slot of their "tiles recomputed last run" counter
      // holds all of their tiles); the probe run every 16th re-measures them
      std::vector<unsigned> seed(3 * (size_t)n, 0u);
      const unsigned nt = (unsigned)inv_tiles(mode, (int)H, (int)W);
      for (int i = 0; i < n; ++i)
        if (params[i].qtable[0] > 60.0) seed[i] = seed[n + i] = seed[2 * (size_t)n + i] = nt;
      if ((e = hipMemcpy((unsigned*)p->invfix.p + 16, seed.data(), sizeof(unsigned) * seed.size(),
                         hipMemcpyHostToDevice)) != hipSuccess) {
        jds_plan_destroy(p);
        return fail(JDS_EHIP, "plan upload: %s", hipGetErrorString(e));
      }
    }
  }
  *out = p;
  return JDS_OK;
}

int jds_plan_fix_counts(const jds_plan* p, uint32_t* counts) {
  if (!p || !counts) return fail(JDS_EINVAL, "null argument");
  // counters[bank n, bank n + n): blocks the last run's k_fix_fwd recomputed, per item;
  // invfix[0]: tiles the last run's certified inverse handed to the exact kernel
  counts[0] = counts[1] = 0u;
  if (p->g.bs == 16) {  // counters[2]: blocks the last certified 16x16 forward recomputed
    hipError_t e = hipDeviceSynchronize();
    if (e == hipSuccess && p->last_fwd16_fast)
      e = hipMemcpy(counts, (const uint32_t*)p->counters.p + 2, 4, hipMemcpyDeviceToHost);
    // and the tiles the last k_inv16_fast run handed to the exact tile body
    if (e == hipSuccess && p->last_inv_fast)
      e = hipMemcpy(counts + 1, (const uint32_t*)p->invfix.p + ((p->inv_runs + 1u) & 1u), 4, hipMemcpyDeviceToHost);
    if (e != hipSuccess) return fail(JDS_EHIP, "fix_counts: %s", hipGetErrorString(e));
    return JDS_OK;
  }
  if (p->g.gen || p->counters.n < 8 * (size_t)p->n) return JDS_OK;
  uint32_t* c = (uint32_t*)malloc(4 * (size_t)p->n + 4);
  if (!c) return fail(JDS_ENOMEM, "fix_counts: host allocation");
  // the last run may be in flight on any stream: wait for the device first
  hipError_t e = hipDeviceSynchronize();
  // single-quality plans: the live counter bank of the last certified run;
  // sweep plans: the list lengths k_fwd_reduce_fix built at [n, 2n)
  const int bank = p->nq > 1 ? 1 : (p->last_fwd8_bank < 0 ? 1 : p->last_fwd8_bank);
  if (e == hipSuccess)
    e = hipMemcpy(c, (const uint32_t*)p->counters.p + bank * p->n, 4 * (size_t)p->n, hipMemcpyDeviceToHost);
  // the last fast-inverse run appended to counter (inv_runs - 1) & 1
  if (e == hipSuccess && p->last_inv_fast)
    e = hipMemcpy(c + p->n, (const uint32_t*)p->invfix.p + ((p->inv_runs + 1u) & 1u), 4, hipMemcpyDeviceToHost);
  if (e != hipSuccess) {
    free(c);
    return fail(JDS_EHIP, "fix_counts: %s", hipGetErrorString(e));
  }
  for (int i = 0; i < p->n; ++i) counts[0] += std::min(c[i], (uint32_t)(p->g.cpf / 64));  // (k_fix_fwd's clamp)
  counts[1] = p->last_inv_fast ? c[p->n] : 0u;
  free(c);
  return JDS_OK;
}

int jds_plan_geometry(const jds_plan* p, jds_geometry* out) {
  if (!p || !out) return fail(JDS_EINVAL, "null argument");
  fill_geometry(p->g, p->mode, out);
  return JDS_OK;
}

int jds_plan_run(jds_plan* p, const uint8_t* rgb, uint8_t* rgb_out, int16_t* coeffs, jds_frame_stats* stats,
                 uint32_t flags, void* stream) {
  if (!p || !rgb || !rgb_out || !coeffs || !stats) return fail(JDS_EINVAL, "null argument");
  if (((uintptr_t)rgb | (uintptr_t)rgb_out | (uintptr_t)coeffs | (uintptr_t)stats) & 15u)
    return fail(JDS_EINVAL, "rgb, rgb_out, coeffs and stats must be 16-byte aligned");
  hipStream_t s = (hipStream_t)stream;  // NULL = the HIP null stream (torch's default stream)
  const MarkScope marks_(p, s);         // jds_plan_profile: launch marks of this run
  int phases = (flags & JDS_RUN_FWD ? 1 : 0) | (flags & JDS_RUN_INV ? 2 : 0);
  if (!phases) phases = 3;
  const bool exact = (flags & JDS_RUN_EXACT) != 0;
  if (p->g.gen) {  // general geometry: exact kernels only (jds_gen.hip)
    if (phases & 1) HIP_TRY(hipMemsetAsync(stats, 0, sizeof(jds_frame_stats) * p->n, s));
    const GenBufs gb = p->gen();
    HIP_TRY(launch_codec(p->mode, p->pf, p->g, p->n, rgb, rgb_out, coeffs, (const FrameQ*)p->fq.p,
                         (const double*)p->gk.p, stats, (double*)p->part.p, (flags & JDS_RUN_SSE) != 0, nullptr,
                         nullptr, nullptr, 0, s, nullptr, phases, p->nq, &gb));
    return JDS_OK;
  }
  if (p->g.bs == 16) {
    // the certified fp32 forward unless JDS_RUN_EXACT (k_fix_fwd16 re-arms its counters)
    const Fwd16Fast ff{p->fq32.p, (const float*)p->gk32.p, (uint32_t*)p->part32.p, (uint2*)p->fixlist.p,
                       (unsigned*)p->counters.p,
                       (flags & JDS_RUN_FWD_FIXALL) ? 1 : 0, (int)(p->fwd16_runs & 1u)};
    if (phases & 1) HIP_TRY(hipMemsetAsync(stats, 0, sizeof(jds_frame_stats) * p->n, s));
    // the certified fast inverse (k_inv16_fast) for 4:2:x runs without SSE
    // terms unless JDS_RUN_EXACT_INV: level with the exact k_inv16s in round 3
    // (524-526 vs 520-522 us at configs[4]), 511 vs 522 us once its certificate
    // reduction went to DPP and its max Q to the host (profiles/r03_v29_ab.txt)
    InvFix fx16 = p->inv_fix();
    fx16.fix_all = (flags & JDS_RUN_INV_FIXALL) ? 1 : 0;
    const bool fast_inv16 = (phases & 2) && !exact && !(flags & JDS_RUN_EXACT_INV) &&
                            !(flags & JDS_RUN_SSE) && p->mode != JDS_SS_444 && p->invfix.p;
    HIP_TRY(launch_codec16(p->mode, p->pf, p->g, p->n, rgb, rgb_out, coeffs, (const FrameQ*)p->fq.p,
                           (const double*)p->gk.p, stats, (double*)p->part.p, (double*)p->planes.p,
                           (flags & JDS_RUN_SSE) != 0, nullptr, nullptr, s, nullptr, phases, exact ? nullptr : &ff,
                           fast_inv16 ? &fx16 : nullptr));
    if (phases & 1) {
      p->last_fwd16_fast = !exact;
      if (!exact) p->fwd16_runs++;
    }
    if (phases & 2) {
      p->last_inv_fast = fast_inv16;
      if (fast_inv16) p->inv_runs++;
    }
    return JDS_OK;
  }
  if (phases & 1) {
    // the fast forward resets the statistics in its front-end launch and
    // re-arms the fix-up counter in k_fwd_reduce (no memsets on its path)
    if (exact) HIP_TRY(hipMemsetAsync(stats, 0, sizeof(jds_frame_stats) * p->n, s));
    if (exact)
      HIP_TRY(launch_codec(p->mode, p->pf, p->g, p->n, rgb, rgb_out, coeffs, (const FrameQ*)p->fq.p,
                           (const double*)p->gk.p, stats, (double*)p->part.p, false, nullptr, nullptr, nullptr, 0,
                           s, nullptr, 1, p->nq, nullptr));
    else
      HIP_TRY(launch_fast_fwd(p->mode, p->pf, p->g, p->n, p->nq, rgb, coeffs, (const FrameQ*)p->fq.p, p->fq32.p,
                              (const double*)p->gk.p, (const float*)p->gk32.p, stats, (uint32_t*)p->part32.p,
                              (uint32_t*)p->fixbits.p, (uint2*)p->fixlist.p, (unsigned*)p->counters.p,
                              (float*)p->dct32.p, s,
                              phases == 1,  // forward + inverse: k_finalize adds the zero bin
                              (int)(p->fwd8_runs & 1u)));
    if (!exact && p->nq == 1) p->last_fwd8_bank = (int)(p->fwd8_runs++ & 1u);
  }
  InvFix fx = p->inv_fix();
  fx.fix_all = (flags & JDS_RUN_INV_FIXALL) ? 1 : 0;
  const bool exact_inv = exact || (flags & JDS_RUN_EXACT_INV) != 0 || (!p->inv_fast_any && !(flags & JDS_RUN_INV_FAST));
  if (phases & 2)
    HIP_TRY(launch_codec(p->mode, p->pf, p->g, p->n, rgb, rgb_out, coeffs, (const FrameQ*)p->fq.p,
                         (const double*)p->gk.p, stats, (double*)p->part.p, (flags & JDS_RUN_SSE) != 0, nullptr,
                         nullptr, nullptr, 0, s, nullptr, exact ? 6 : (phases == 3 ? 2 | 8 : 2), p->nq, nullptr,
                         exact_inv || !p->invfix.p ? nullptr : &fx));
  if (phases & 2) {
    p->last_inv_fast = !exact_inv && p->invfix.p;
    if (p->last_inv_fast) p->inv_runs++;
  }
  return JDS_OK;
}

// The launch marks of a plan or of a context (jds_plan_profile, jds_ctx_profile).
static int marks_enable(KMarks& marks, bool& on, int device, int enable) {
  if (enable && !marks.cap) {
    HIP_TRY(hipSetDevice(device));
    const int cap = 8192;  // marks until the next read: ~7 per run
    KMarks m;
    m.ev = (hipEvent_t*)calloc(cap, sizeof(hipEvent_t));
    m.name = (char(*)[64])calloc(cap, sizeof *m.name);
    if (!m.ev || !m.name) {
      free(m.ev);
      free(m.name);
      return fail(JDS_ENOMEM, "host allocation failed");
    }
    for (; m.cap < cap; ++m.cap) {
      // timing-only marks: no system-scope fence (cache write-back and
      // invalidate) per mark, which otherwise lands inside the next launch's
      // interval and perturbs the profiled step (r06: +5 % over the timed one)
      hipError_t e = hipEventCreateWithFlags(&m.ev[m.cap], hipEventDisableSystemFence);
      if (e != hipSuccess) {
        marks_release(m);
        return fail(JDS_EHIP, "hipEventCreate: %s", hipGetErrorString(e));
      }
    }
    marks = m;
  }
  on = enable != 0;
  marks.n = 0;
  marks.dropped = 0;
  return JDS_OK;
}

int jds_plan_profile(jds_plan* p, int enable) {
  if (!p) return fail(JDS_EINVAL, "null argument");
  return marks_enable(p->marks, p->prof_on, p->ctx->device, enable);
}

static int marks_read(KMarks& m, int device, jds_kernel_time* out, int max, int* n_out, double* span_ms) {
  if (!n_out || (max > 0 && !out)) return fail(JDS_EINVAL, "null argument");
  *n_out = 0;
  if (span_ms) *span_ms = 0.0;
  if (m.dropped) {  // the pool filled up: partial totals would under-report, so none are returned
    const long long d = m.dropped;
    if (m.n) (void)hipEventSynchronize(m.ev[m.n - 1]);
    m.n = 0;
    m.dropped = 0;
    return fail(JDS_EINVAL, "profile overflow: %lld launch marks dropped (pool of %d); read every <= %d runs",
                d, m.cap, m.cap / 8);
  }
  if (m.n < 2) {
    m.n = 0;
    return JDS_OK;
  }
  HIP_TRY(hipSetDevice(device));
  HIP_TRY(hipEventSynchronize(m.ev[m.n - 1]));
  int k = 0;
  for (int i = 1; i < m.n; ++i) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, m.ev[i - 1], m.ev[i]));
    int j = 0;
    while (j < k && strncmp(out[j].name, m.name[i], sizeof out[j].name) != 0) ++j;
    if (j == k) {
      if (k == max) continue;  // more distinct names than the caller's array holds
      memset(&out[k], 0, sizeof out[k]);
      snprintf(out[k].name, sizeof out[k].name, "%s", m.name[i]);
      ++k;
    }
    out[j].total_ms += ms;
    out[j].launches += 1;
  }
  if (span_ms) {
    float ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&ms, m.ev[0], m.ev[m.n - 1]));
    *span_ms = ms;
  }
  *n_out = k;
  m.n = 0;
  return JDS_OK;
}

int jds_plan_profile_read(jds_plan* p, jds_kernel_time* out, int max, int* n_out, double* span_ms) {
  if (!p) return fail(JDS_EINVAL, "null argument");
  return marks_read(p->marks, p->ctx->device, out, max, n_out, span_ms);
}

int jds_ctx_profile(jds_ctx* c, int enable) {
  if (!c) return fail(JDS_EINVAL, "null argument");
  return marks_enable(c->marks, c->prof_on, c->device, enable);
}

int jds_ctx_profile_read(jds_ctx* c, jds_kernel_time* out, int max, int* n_out, double* span_ms) {
  if (!c) return fail(JDS_EINVAL, "null argument");
  return marks_read(c->marks, c->device, out, max, n_out, span_ms);
}

void jds_plan_destroy(jds_plan* p) {
  if (!p) return;
  (void)hipSetDevice(p->ctx->device);
  (void)hipStreamSynchronize(p->ctx->stream);
  p->fq.release();
  p->gk.release();
  p->part.release();
  p->fq32.release();
  p->gk32.release();
  p->fixlist.release();
  p->counters.release();
  p->fixbits.release();
  p->part32.release();
  p->invfix.release();
  p->invlist.release();
  p->planes.release();
  p->dct32.release();
  p->gen_tab.release();
  p->gen_sub.release();
  p->gen_rec.release();
  for (DevBuf& b : p->ent) b.release();
  p->ent_hdr.release();
  p->ent_tab.release();
  p->dec_tab.release();
  p->dec_scr.release();
  p->dec_info.release();
  p->rst_hdr.release();
  p->rst_work.release();
  free(p->qt);
  marks_release(p->marks);
  delete p;
}

int jds_compress_reconstruct(jds_ctx* c, const jds_params* prm, const uint8_t* rgb, int64_t H, int64_t W,
                             uint8_t* rgb_out, int16_t* coeffs, jds_frame_stats* stats, double* error_map_y,
                             double* error_map_rgb, int32_t sel_by, int32_t sel_bx, jds_selected_block* sel,
                             int32_t* sel_valid) {
  if (!c || !prm || !rgb || !rgb_out || !stats) return fail(JDS_EINVAL, "null argument");
  if ((error_map_y == nullptr) != (error_map_rgb == nullptr))
    return fail(JDS_EINVAL, "error_map_y and error_map_rgb must be requested together");
  Geo g;
  int mode;
  bool pf;
  int rc = make_geo(prm, H, W, &g, &mode, &pf);
  if (rc) return rc;
  if ((rc = check_tables(prm))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t npx = (size_t)H * (size_t)W, nimg = npx * 3, ncf = (size_t)g.cpf;
  const int tiles = std::max(std::max(g.tiles_y * g.tiles_x, g.gen ? gen_px_tiles(g) : 0),
                             g.bs == 16 ? inv16_tiles(mode, (int)H, (int)W) : 0);
  HIP_TRY(c->rgb.ensure(nimg));
  HIP_TRY(c->out.ensure(nimg));
  HIP_TRY(c->coeffs.ensure(ncf * sizeof(int16_t)));
  HIP_TRY(c->stats.ensure(sizeof(jds_frame_stats)));
  HIP_TRY(c->part.ensure(sizeof(double) * tiles));
  HIP_TRY(c->fq.ensure(sizeof(FrameQ)));
  HIP_TRY(c->gk.ensure(3 * sizeof(double)));
  const bool maps = error_map_y != nullptr;
  if (maps) {
    HIP_TRY(c->erry.ensure(npx * sizeof(double)));
    HIP_TRY(c->errrgb.ensure(npx * sizeof(double)));
  }
  // selected luma block (pipeline.py:132-138): index into the padded grid
  // (8x8 only: jds_selected_block holds 8x8 arrays; the 16x16 path reports none)
  int sel_blk = -1;
  if (sel && g.bs == 16) {
    if (sel_valid) *sel_valid = 0;
  } else if (sel) {
    const long long bpr = g.nbx;
    const long long ti = (long long)sel_by * bpr + sel_bx;
    const long long nyb = (long long)g.nby * g.nbx;
    if (ti >= 0 && ti < nyb) sel_blk = (int)ti;
    if (sel_valid) *sel_valid = sel_blk >= 0;
    if (sel_blk >= 0) HIP_TRY(c->sel.ensure(sizeof(jds_selected_block)));
  }
  FrameQ hq;
  make_fq(prm, &hq);
  hipStream_t s = c->stream;
  GenBufs gb{};
  if (g.gen) {
    if ((rc = gen_prepare(g, 1, 1, c->gen_tab, c->gen_sub, c->gen_rec, s))) return rc;
    gb = {(const AreaTap*)c->gen_tab.p, (double*)c->gen_sub.p, (double*)c->gen_rec.p};
  }
  HIP_TRY(hipMemcpyAsync(c->fq.p, &hq, sizeof hq, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->gk.p, prm->gauss, 3 * sizeof(double), hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->rgb.p, rgb, nimg, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(c->stats.p, 0, sizeof(jds_frame_stats), s));
  jds_selected_block* dsel = sel_blk >= 0 ? (jds_selected_block*)c->sel.p : nullptr;
  if (g.bs == 16) {
    HIP_TRY(c->planes.ensure(sizeof(double) * 2 * (size_t)g.hc * g.wc));
    HIP_TRY(launch_codec16(mode, pf, g, 1, (const uint8_t*)c->rgb.p, (uint8_t*)c->out.p, (int16_t*)c->coeffs.p,
                           (const FrameQ*)c->fq.p, (const double*)c->gk.p, (jds_frame_stats*)c->stats.p,
                           (double*)c->part.p, (double*)c->planes.p, true, maps ? (double*)c->erry.p : nullptr,
                           maps ? (double*)c->errrgb.p : nullptr, s, c->ev, 3, nullptr, nullptr));
  } else
  HIP_TRY(launch_codec(mode, pf, g, 1, (const uint8_t*)c->rgb.p, (uint8_t*)c->out.p, (int16_t*)c->coeffs.p,
                       (const FrameQ*)c->fq.p, (const double*)c->gk.p, (jds_frame_stats*)c->stats.p,
                       (double*)c->part.p, true, maps ? (double*)c->erry.p : nullptr,
                       maps ? (double*)c->errrgb.p : nullptr, dsel, sel_blk, s, c->ev, 3, 1, &gb));
  // the outputs are final here: their copies to the caller's (pageable) arrays
  // go on the transfer stream, so the statistics kernels queued below on `s`
  // run while the host thread stages the copies
  if (!c->xfer) {
    HIP_TRY(hipStreamCreateWithFlags(&c->xfer, hipStreamNonBlocking));
    HIP_TRY(hipEventCreateWithFlags(&c->xfer_ev, hipEventDisableTiming));
  }
  HIP_TRY(hipEventRecord(c->xfer_ev, s));
  HIP_TRY(hipStreamWaitEvent(c->xfer, c->xfer_ev, 0));
  {
    // NumPy float32 magnitude_bits (utils/metrics.py:77-78)
    const long long nblk = g.cpf / 64;
    const int max_chunks = (int)((g.cpf + 8191) / 8192) + 1;
    HIP_TRY(c->chunks.ensure(mag_scratch_bytes(nblk, max_chunks)));
    HIP_TRY(launch_mag_f32((const int16_t*)c->coeffs.p, nblk, (unsigned*)c->chunks.p, max_chunks,
                           &((jds_frame_stats*)c->stats.p)->magnitude_bits_f32, s));
  }
  if (H >= 7 && W >= 7) {
    jds_frame_stats* dst = (jds_frame_stats*)c->stats.p;
    if ((rc = run_ssim(c, (const uint8_t*)c->rgb.p, (const uint8_t*)c->out.p, (int)H, (int)W, &dst->ssim[0])))
      return rc;
  }
  hipStream_t x = c->xfer;
  // every exit from here on waits for the copies queued on x: an error return
  // must not leave copies into the caller's arrays in flight
  struct XferWait {
    hipStream_t x;
    ~XferWait() { (void)hipStreamSynchronize(x); }
  } xfer_wait{x};
  HIP_TRY(hipMemcpyAsync(rgb_out, c->out.p, nimg, hipMemcpyDeviceToHost, x));
  if (coeffs) HIP_TRY(hipMemcpyAsync(coeffs, c->coeffs.p, ncf * sizeof(int16_t), hipMemcpyDeviceToHost, x));
  if (maps) {
    HIP_TRY(hipMemcpyAsync(error_map_y, c->erry.p, npx * sizeof(double), hipMemcpyDeviceToHost, x));
    HIP_TRY(hipMemcpyAsync(error_map_rgb, c->errrgb.p, npx * sizeof(double), hipMemcpyDeviceToHost, x));
  }
  if (dsel) HIP_TRY(hipMemcpyAsync(sel, dsel, sizeof(jds_selected_block), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(stats, c->stats.p, sizeof(jds_frame_stats), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(x));
  HIP_TRY(hipStreamSynchronize(s));
  if (!(H >= 7 && W >= 7)) {
    for (int i = 0; i < 4; ++i) stats->ssim[i] = __builtin_nan("");
    stats->mse_y = __builtin_nan("");
  }
  float t0 = 0.f, t1 = 0.f;
  HIP_TRY(hipEventElapsedTime(&t0, c->ev[0], c->ev[1]));
  HIP_TRY(hipEventElapsedTime(&t1, c->ev[1], c->ev[2]));
  stats->fwd_ms = t0;
  stats->inv_ms = t1;
  return JDS_OK;
}

// jds_psnr_ssim / jds_psnr_ssim_dev: argument checks shared by both
static int psnr_ssim_args(jds_ctx* c, const uint8_t* a, const uint8_t* b, int64_t H, int64_t W, double* out) {
  if (!c || !a || !b || !out) return fail(JDS_EINVAL, "null argument");
  if (H < 7 || W < 7)
    return fail(JDS_EINVAL,
                "win_size exceeds image extent. Either ensure that your images are at least 7x7; or pass "
                "win_size explicitly in the function call, with an odd value less than or equal to the "
                "smaller side of your images. If your images are multichannel (with color channels), set "
                "channel_axis to the axis number corresponding to the channels.");
  if (H * W > (int64_t)1 << 28) return fail(JDS_EINVAL, "image too large");
  return JDS_OK;
}

// SSIM / MSE of `items` device-resident image pairs (the context's stream):
// out[6 i + 0..5] = SSIM R, G, B, Y, MSE Y, MSE RGB on the host
static int psnr_ssim_device_batch(jds_ctx* c, int items, const uint8_t* const* a, const uint8_t* const* b,
                                  int64_t H, int64_t W, double* out) {
  const size_t nb = (size_t)H * W * 3;
  const size_t bytes = (size_t)items * (5 * sizeof(double) + sizeof(unsigned long long));
  HIP_TRY(c->ss_out.ensure(bytes));
  hipStream_t s = c->stream;
  double* dres = (double*)c->ss_out.p;
  unsigned long long* dsse = (unsigned long long*)(dres + (size_t)5 * items);
  int rc = run_ssim_batch(c, items, a, b, (int)H, (int)W, dres, 5, dsse);
  if (rc) return rc;
  double* res = (double*)malloc(bytes);
  if (!res) return fail(JDS_ENOMEM, "host allocation failed");
  hipError_t e = hipMemcpyAsync(res, dres, bytes, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  if (e != hipSuccess) {
    free(res);
    return fail(JDS_EHIP, "HIP error: %s", hipGetErrorString(e));
  }
  const unsigned long long* sse = (const unsigned long long*)(res + (size_t)5 * items);
  for (int i = 0; i < items; ++i) {
    for (int k = 0; k < 5; ++k) out[6 * i + k] = res[5 * i + k];
    out[6 * i + 5] = (double)sse[i] / (double)nb;  // exact: integer sum, one division (np.mean)
  }
  free(res);
  return JDS_OK;
}

static int psnr_ssim_device(jds_ctx* c, const uint8_t* a, const uint8_t* b, int64_t H, int64_t W, double* out) {
  return psnr_ssim_device_batch(c, 1, &a, &b, H, W, out);
}

int jds_psnr_ssim(jds_ctx* c, const uint8_t* a, const uint8_t* b, int64_t H, int64_t W, double* out) {
  int rc = psnr_ssim_args(c, a, b, H, W, out);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nb = (size_t)H * W * 3;
  HIP_TRY(c->img_a.ensure(nb));
  HIP_TRY(c->img_b.ensure(nb));
  HIP_TRY(hipMemcpyAsync(c->img_a.p, a, nb, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(hipMemcpyAsync(c->img_b.p, b, nb, hipMemcpyHostToDevice, c->stream));
  return psnr_ssim_device(c, (const uint8_t*)c->img_a.p, (const uint8_t*)c->img_b.p, H, W, out);
}

int jds_psnr_ssim_dev(jds_ctx* c, const uint8_t* a_dev, const uint8_t* b_dev, int64_t H, int64_t W, double* out) {
  int rc = psnr_ssim_args(c, a_dev, b_dev, H, W, out);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(hipDeviceSynchronize());  // the images come from other streams (plan runs, torch)
  return psnr_ssim_device(c, a_dev, b_dev, H, W, out);
}

// the context's stream waits for what `after` has queued so far (one event);
// JDS_AFTER_NONE: no wait (the caller has synchronised); NULL: the HIP null stream
static int wait_after(jds_ctx* c, void* after) {
  if (after == JDS_AFTER_NONE) return JDS_OK;
  hipEvent_t e;
  HIP_TRY(hipEventCreateWithFlags(&e, hipEventDisableTiming));
  hipError_t err = hipEventRecord(e, (hipStream_t)after);
  if (err == hipSuccess) err = hipStreamWaitEvent(c->stream, e, 0);
  hipError_t d = hipEventDestroy(e);  // released once the wait has completed
  if (err != hipSuccess) return fail(JDS_EHIP, "HIP error: %s", hipGetErrorString(err));
  if (d != hipSuccess) return fail(JDS_EHIP, "HIP error: %s", hipGetErrorString(d));
  return JDS_OK;
}

int jds_psnr_ssim_dev_after(jds_ctx* c, const uint8_t* a_dev, const uint8_t* b_dev, int64_t H, int64_t W,
                            double* out, void* after) {
  int rc = psnr_ssim_args(c, a_dev, b_dev, H, W, out);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = wait_after(c, after))) return rc;
  return psnr_ssim_device(c, a_dev, b_dev, H, W, out);
}

int jds_psnr_ssim_batch_dev(jds_ctx* c, int32_t n, const uint8_t* const* a_dev, const uint8_t* const* b_dev, int64_t H,
                            int64_t W, double* out, void* after) {
  if (!c || n < 0 || (n > 0 && (!a_dev || !b_dev || !out))) return fail(JDS_EINVAL, "null argument");
  if (n == 0) return JDS_OK;
  for (int i = 0; i < n; ++i) {
    int rc = psnr_ssim_args(c, a_dev[i], b_dev[i], H, W, out);
    if (rc) return rc;
  }
  HIP_TRY(hipSetDevice(c->device));
  int rc = wait_after(c, after);
  if (rc) return rc;
  return psnr_ssim_device_batch(c, n, a_dev, b_dev, H, W, out);
}

int jds_magnitude_bits_f32_batch_dev(jds_ctx* c, const int16_t* coeffs_dev, int32_t n_items, int64_t n_coeffs,
                                     int64_t item_stride, double* out, void* after) {
  if (!c || n_items < 0 || (n_items > 0 && (!coeffs_dev || !out)) || n_coeffs < 0 || n_coeffs % 64 ||
      item_stride < n_coeffs)
    return fail(JDS_EINVAL, "bad argument");
  if (n_coeffs > ((int64_t)1 << 31)) return fail(JDS_EINVAL, "too many coefficients");
  if (n_items == 0) return JDS_OK;
  HIP_TRY(hipSetDevice(c->device));
  int rc = wait_after(c, after);
  if (rc) return rc;
  hipStream_t s = c->stream;
  const long long nblk = n_coeffs / 64;
  const int max_chunks = (int)((n_coeffs + 8191) / 8192) + 1;
  HIP_TRY(c->chunks.ensure(mag_scratch_bytes(nblk, max_chunks)));
  HIP_TRY(c->ss_out.ensure(sizeof(double) * (size_t)n_items));
  double* d = (double*)c->ss_out.p;
  // one launch chain per item on the stream (the scratch is reused in order), one copy, one wait
  for (int i = 0; i < n_items; ++i)
    HIP_TRY(launch_mag_f32(coeffs_dev + (size_t)i * item_stride, nblk, (unsigned*)c->chunks.p, max_chunks, d + i, s));
  HIP_TRY(hipMemcpyAsync(out, d, sizeof(double) * (size_t)n_items, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return JDS_OK;
}

int jds_magnitude_bits_f32_dev(jds_ctx* c, const int16_t* coeffs_dev, int64_t n_coeffs, double* out, void* after) {
  if (!c || !coeffs_dev || !out || n_coeffs < 0 || n_coeffs % 64) return fail(JDS_EINVAL, "bad argument");
  if (n_coeffs > ((int64_t)1 << 31)) return fail(JDS_EINVAL, "too many coefficients");
  HIP_TRY(hipSetDevice(c->device));
  int rc = wait_after(c, after);
  if (rc) return rc;
  hipStream_t s = c->stream;
  const long long nblk = n_coeffs / 64;
  const int max_chunks = (int)((n_coeffs + 8191) / 8192) + 1;
  HIP_TRY(c->chunks.ensure(mag_scratch_bytes(nblk, max_chunks)));
  HIP_TRY(c->ss_out.ensure(5 * sizeof(double) + sizeof(unsigned long long)));
  double* d = (double*)c->ss_out.p;
  HIP_TRY(launch_mag_f32(coeffs_dev, nblk, (unsigned*)c->chunks.p, max_chunks, d, s));
  HIP_TRY(hipMemcpyAsync(out, d, sizeof(double), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return JDS_OK;
}

// ----------------------------------------------------- per-stage API --

static int stage_io(jds_ctx* c, int idx, const void* host, size_t bytes, void** dev) {
  HIP_TRY(c->st[idx].ensure(bytes));
  if (host) HIP_TRY(hipMemcpyAsync(c->st[idx].p, host, bytes, hipMemcpyHostToDevice, c->stream));
  *dev = c->st[idx].p;
  return JDS_OK;
}

static int stage_out(jds_ctx* c, void* host, const void* dev, size_t bytes) {
  HIP_TRY(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return JDS_OK;
}

static int stage_rgb(jds_ctx* c, const double* in, double* out, int64_t n, int inverse) {
  if (!c || !in || !out || n < 0) return fail(JDS_EINVAL, "bad argument");
  if (n == 0) return JDS_OK;
  HIP_TRY(hipSetDevice(c->device));
  void *di, *dout;
  int rc;
  const size_t b = (size_t)n * 3 * sizeof(double);
  if ((rc = stage_io(c, 0, in, b, &di)) || (rc = stage_io(c, 1, nullptr, b, &dout))) return rc;
  HIP_TRY(stage_rgb_ycc((const double*)di, (double*)dout, n, inverse, c->stream));
  return stage_out(c, out, dout, b);
}

int jds_stage_rgb_to_ycbcr(jds_ctx* c, const double* rgb, double* ycc, int64_t n_pixels) {
  return stage_rgb(c, rgb, ycc, n_pixels, 0);
}

int jds_stage_ycbcr_to_rgb(jds_ctx* c, const double* ycc, double* rgb, int64_t n_pixels) {
  return stage_rgb(c, ycc, rgb, n_pixels, 1);
}

int jds_stage_subsample(jds_ctx* c, const double* cb, const double* cr, int64_t H, int64_t W, int32_t mode,
                        int32_t prefilter, const double* gauss, double* cb_out, double* cr_out) {
  if (!c || !cb || !cr || !cb_out || !cr_out || !gauss || H < 1 || W < 1) return fail(JDS_EINVAL, "bad argument");
  if (mode != JDS_SS_422 && mode != JDS_SS_420) return fail(JDS_EINVAL, "Unknown subsampling mode: %d", mode);
  const int sy = mode == JDS_SS_420 ? 2 : 1;
  const int oh = (int)(H / sy), ow = (int)(W / 2);
  if (oh < 1 || ow < 1)
    return fail(JDS_EINVAL,
                "OpenCV(4.8.0) resize.cpp: error: (-215:Assertion failed) !dsize.empty() in function 'resize'");
  // odd sizes take cv2's fractional INTER_AREA path (tables as in jds_gen.hip)
  const bool gen = (W % 2) || (sy == 2 && (H % 2));
  HIP_TRY(hipSetDevice(c->device));
  const size_t n = (size_t)H * W, bi = n * sizeof(double), bo = (size_t)oh * ow * sizeof(double);
  void *din, *t1, *t2, *dout;
  int rc;
  if ((rc = stage_io(c, 1, nullptr, bi, &t1)) || (rc = stage_io(c, 2, nullptr, bi, &t2)) ||
      (rc = stage_io(c, 3, nullptr, bo, &dout)))
    return rc;
  if (gen) {
    Geo g{};
    g.H = (int)H;
    g.W = (int)W;
    g.hc = oh;
    g.wc = ow;
    if ((rc = gen_prepare(g, 0, 0, c->gen_tab, c->gen_sub, c->gen_rec, c->stream))) return rc;
  }
  const double* planes[2] = {cb, cr};
  double* outs[2] = {cb_out, cr_out};
  for (int p = 0; p < 2; ++p) {
    if ((rc = stage_io(c, 0, planes[p], bi, &din))) return rc;
    if (gen) {
      // blur (if any) as the fast path does, then the fractional area resize
      const double* src = (const double*)din;
      if (prefilter) {
        HIP_TRY(stage_subsample((const double*)din, (double*)t1, (double*)t2, nullptr, (int)H, (int)W, sy, 1, gauss,
                                c->stream));
        src = (const double*)t2;
      }
      const AreaTap* tabs = (const AreaTap*)c->gen_tab.p;
      HIP_TRY(stage_area_gen(src, (int)H, (int)W, tabs, tabs + oh, (double*)dout, oh, ow, c->stream));
    } else {
      HIP_TRY(stage_subsample((const double*)din, (double*)t1, (double*)t2, (double*)dout, (int)H, (int)W, sy,
                              prefilter, gauss, c->stream));
    }
    if ((rc = stage_out(c, outs[p], dout, bo))) return rc;
  }
  return JDS_OK;
}

int jds_stage_upsample(jds_ctx* c, const double* in, int64_t h, int64_t w, int64_t H, int64_t W, int32_t nearest,
                       double* out) {
  if (!c || !in || !out || h < 1 || w < 1 || H < 1 || W < 1) return fail(JDS_EINVAL, "bad argument");
  HIP_TRY(hipSetDevice(c->device));
  void *din, *dout;
  int rc;
  if ((rc = stage_io(c, 0, in, (size_t)h * w * sizeof(double), &din)) ||
      (rc = stage_io(c, 1, nullptr, (size_t)H * W * sizeof(double), &dout)))
    return rc;
  HIP_TRY(stage_resize((const double*)din, (int)h, (int)w, (double*)dout, (int)H, (int)W, nearest, c->stream));
  return stage_out(c, out, dout, (size_t)H * W * sizeof(double));
}

int jds_stage_block_dct_n(jds_ctx* c, const double* in, double* out, int64_t n_blocks, int32_t block_size,
                          int32_t op) {
  if (!c || !in || !out || n_blocks < 0 || op < 0 || op > 3) return fail(JDS_EINVAL, "bad argument");
  if (block_size != 8 && block_size != 16)
    return fail(JDS_ENOTSUP, "block transforms are 8x8 or 16x16 (got %d)", block_size);
  if (n_blocks == 0) return JDS_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t b = (size_t)n_blocks * block_size * block_size * sizeof(double);
  void *din, *dout;
  int rc;
  if ((rc = stage_io(c, 0, in, b, &din)) || (rc = stage_io(c, 1, nullptr, b, &dout))) return rc;
  HIP_TRY(stage_block((const double*)din, (double*)dout, n_blocks, block_size, op, c->stream));
  return stage_out(c, out, dout, b);
}

int jds_stage_block_dct(jds_ctx* c, const double* in, double* out, int64_t n_blocks, int32_t op) {
  return jds_stage_block_dct_n(c, in, out, n_blocks, 8, op);
}

int jds_stage_quantize_n(jds_ctx* c, const void* in, const double* qtable, int32_t table_len, void* out, int64_t n,
                         int32_t dequant) {
  if (!c || !in || !qtable || !out || n < 0) return fail(JDS_EINVAL, "bad argument");
  if ((table_len != 64 && table_len != 256) || (n % table_len)) return fail(JDS_EINVAL, "bad table length");
  if (n == 0) return JDS_OK;
  HIP_TRY(hipSetDevice(c->device));
  const size_t bi = (size_t)n * (dequant ? sizeof(int16_t) : sizeof(double));
  const size_t bo = (size_t)n * (dequant ? sizeof(double) : sizeof(int16_t));
  void *din, *dq, *dout;
  int rc;
  if ((rc = stage_io(c, 0, in, bi, &din)) || (rc = stage_io(c, 4, qtable, table_len * sizeof(double), &dq)) ||
      (rc = stage_io(c, 1, nullptr, bo, &dout)))
    return rc;
  HIP_TRY(stage_quant(din, (const double*)dq, dout, n, dequant, table_len, c->stream));
  return stage_out(c, out, dout, bo);
}

int jds_stage_quantize(jds_ctx* c, const void* in, const double* qtable, void* out, int64_t n, int32_t dequant) {
  return jds_stage_quantize_n(c, in, qtable, 64, out, n, dequant);
}

// ------------------------------------------------------- entropy coding --

// Entropy-coder scratch for n frames of geometry g, plus per-frame JFIF headers
// built from the 8x8 tables qt (n x 64).
static int ent_prepare(const Geo& g, int mode, int n, const double* qt, DevBuf* ent, DevBuf& hdr, DevBuf& tab,
                       hipStream_t s) {
  if (g.bs != 8) return fail(JDS_ENOTSUP, "JPEG entropy coding needs 8x8 blocks (block_size %d)", g.bs);
  if (g.H > 65535 || g.W > 65535) return fail(JDS_ENOTSUP, "baseline JPEG is limited to 65535 x 65535");
  if (g.gen) {
    // T.81 sizes a subsampled component ceil(W/2) x ceil(H/sy); the reference's
    // planes are floor-sized (cv2.resize).  The scans are valid only when both
    // give the same block grid.
    const int sy = mode == JDS_SS_420 ? 2 : 1;
    const int jw = (g.W + 1) / 2, jh = (g.H + sy - 1) / sy;
    if ((jw + 7) / 8 != g.ncx || (jh + 7) / 8 != g.ncy)
      return fail(JDS_ENOTSUP, "%dx%d: the chroma block grid (%dx%d) differs from baseline JPEG's (%dx%d)", g.H,
                  g.W, g.ncy, g.ncx, (jh + 7) / 8, (jw + 7) / 8);
  }
  size_t sz[8];
  ent_sizes(g, n, sz);
  for (int i = 0; i < 8; ++i)
    if (i != 6) HIP_TRY(ent[i].ensure(sz[i]));
  const size_t hl = sz[6] / (size_t)n;
  uint8_t* h = (uint8_t*)malloc(sz[6]);
  if (!h) return fail(JDS_ENOMEM, "host allocation failed");
  for (int i = 0; i < n; ++i) {
    if (ent_header(qt + 64 * i, mode, g.H, g.W, h + hl * i) != (int)hl) {
      free(h);
      return fail(JDS_EINVAL, "frame %d: baseline JPEG needs integer quantisation steps in [1, 255]", i);
    }
  }
  hipError_t e = hdr.ensure(sz[6]);
  if (e == hipSuccess) e = hipMemcpyAsync(hdr.p, h, sz[6], hipMemcpyHostToDevice, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);  // h is freed below
  free(h);
  HIP_TRY(e);
  if (!tab.p) {
    alignas(16) static thread_local char t[16384];
    if (ent_tab_size() > sizeof t) return fail(JDS_EINVAL, "entropy tables exceed the staging buffer");
    ent_build_tables((EntTab*)t);
    HIP_TRY(tab.ensure(ent_tab_size()));
    HIP_TRY(hipMemcpy(tab.p, t, ent_tab_size(), hipMemcpyHostToDevice));
  }
  return JDS_OK;
}

int jds_plan_entropy_capacity(const jds_plan* p, int64_t* bytes_per_frame) {
  if (!p || !bytes_per_frame) return fail(JDS_EINVAL, "null argument");
  if (p->g.bs != 8) return fail(JDS_ENOTSUP, "JPEG entropy coding needs 8x8 blocks (block_size %d)", p->g.bs);
  *bytes_per_frame = ent_capacity(p->g);
  return JDS_OK;
}

// The writer's restart interval: 0 is the plain calls' business, anything but the coder's segment size unsupported.
static int check_writer_interval(int32_t interval) {
  if (interval == 0)
    return fail(JDS_EINVAL, "restart interval 0: the plain entropy calls write files without restart markers");
  if (interval != ent_restart_interval())
    return fail(JDS_ENOTSUP, "restart interval %d: the writer supports %d (its segment size) and 0", interval,
                ent_restart_interval());
  return JDS_OK;
}

static int plan_entropy(jds_plan* p, bool rst, const int16_t* coeffs, uint8_t* out, int64_t out_stride,
                        uint64_t* lengths, uint64_t* scan_bits, void* stream, bool opt = false) {
  if (!p || !coeffs || !out || !lengths) return fail(JDS_EINVAL, "null argument");
  if (p->g.bs != 8) return fail(JDS_ENOTSUP, "JPEG entropy coding needs 8x8 blocks (block_size %d)", p->g.bs);
  const long long cap = opt ? ent_capacity_opt(p->g, rst) : (rst ? ent_capacity_rst(p->g) : ent_capacity(p->g));
  if (out_stride < cap)
    return fail(JDS_EINVAL, "out_stride %lld < worst-case file size %lld", (long long)out_stride, cap);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (!p->ent_hdr.p) {
    int rc = ent_prepare(p->g, p->mode, p->n, p->qt, p->ent, p->ent_hdr, p->ent_tab, s);
    if (rc) return rc;
  }
  void* bufs[8];
  for (int i = 0; i < 8; ++i) bufs[i] = p->ent[i].p;
  const MarkScope marks_(p, s);
  auto* launch = opt ? (rst ? launch_entropy_rst_opt : launch_entropy_opt)
                     : (rst ? launch_entropy_rst : launch_entropy);
  HIP_TRY(launch(p->g, p->n, coeffs, bufs, (const uint8_t*)p->ent_hdr.p, p->ent_tab.p, out, out_stride,
                 (unsigned long long*)lengths, (unsigned long long*)scan_bits, s));
  return JDS_OK;
}

int jds_plan_entropy(jds_plan* p, const int16_t* coeffs, uint8_t* out, int64_t out_stride, uint64_t* lengths,
                     uint64_t* scan_bits, void* stream) {
  return plan_entropy(p, false, coeffs, out, out_stride, lengths, scan_bits, stream);
}

int jds_entropy_restart_info(int32_t* writer_interval, int32_t* lane_max_blocks) {
  if (!writer_interval || !lane_max_blocks) return fail(JDS_EINVAL, "null argument");
  int lm;
  rst_constants(&lm);
  *writer_interval = ent_restart_interval();
  *lane_max_blocks = lm;
  return JDS_OK;
}

int jds_plan_entropy_capacity_rst(const jds_plan* p, int32_t interval, int64_t* bytes_per_frame) {
  if (!p || !bytes_per_frame) return fail(JDS_EINVAL, "null argument");
  if (p->g.bs != 8) return fail(JDS_ENOTSUP, "JPEG entropy coding needs 8x8 blocks (block_size %d)", p->g.bs);
  const int rc = check_writer_interval(interval);
  if (rc) return rc;
  *bytes_per_frame = ent_capacity_rst(p->g);
  return JDS_OK;
}

int jds_plan_entropy_rst(jds_plan* p, int32_t interval, const int16_t* coeffs, uint8_t* out, int64_t out_stride,
                         uint64_t* lengths, uint64_t* scan_bits, void* stream) {
  const int rc = check_writer_interval(interval);
  if (rc) return rc;
  return plan_entropy(p, true, coeffs, out, out_stride, lengths, scan_bits, stream);
}

static int encode_jfif(jds_ctx* c, const jds_params* prm, int64_t H, int64_t W, bool rst, const int16_t* coeffs,
                       uint8_t* out, int64_t out_cap, int64_t* out_len, uint64_t* scan_bits, bool opt = false) {
  if (!c || !prm || !coeffs || !out || !out_len) return fail(JDS_EINVAL, "null argument");
  Geo g;
  int mode;
  int rc = make_geo(prm, H, W, &g, &mode, nullptr);
  if (rc) return rc;
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  if ((rc = ent_prepare(g, mode, 1, prm->qtable, c->ent, c->ent_hdr, c->ent_tab, s))) return rc;
  const long long cap = opt ? ent_capacity_opt(g, rst) : (rst ? ent_capacity_rst(g) : ent_capacity(g));
  HIP_TRY(c->ent_cf.ensure((size_t)g.cpf * sizeof(int16_t)));
  HIP_TRY(c->ent_out.ensure((size_t)cap));
  HIP_TRY(c->ent_meta.ensure(4 * sizeof(unsigned long long)));
  HIP_TRY(hipMemcpyAsync(c->ent_cf.p, coeffs, (size_t)g.cpf * sizeof(int16_t), hipMemcpyHostToDevice, s));
  void* bufs[8];
  for (int i = 0; i < 8; ++i) bufs[i] = c->ent[i].p;
  unsigned long long* meta = (unsigned long long*)c->ent_meta.p;
  auto* launch = opt ? (rst ? launch_entropy_rst_opt : launch_entropy_opt)
                     : (rst ? launch_entropy_rst : launch_entropy);
  HIP_TRY(launch(g, 1, (const int16_t*)c->ent_cf.p, bufs, (const uint8_t*)c->ent_hdr.p, c->ent_tab.p,
                 (uint8_t*)c->ent_out.p, cap, meta, meta + 1, s));
  unsigned long long m[4];
  HIP_TRY(hipMemcpyAsync(m, meta, sizeof m, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  if (m[0] == 0)
    return fail(JDS_EINVAL, "coefficients outside baseline JPEG's range (DC difference category > 11 or "
                            "AC category > 10)");
  *out_len = (int64_t)m[0];
  if (scan_bits)
    for (int i = 0; i < 3; ++i) scan_bits[i] = m[1 + i];
  if ((long long)m[0] > out_cap) return fail(JDS_EINVAL, "output buffer too small: %llu bytes needed", m[0]);
  HIP_TRY(hipMemcpy(out, c->ent_out.p, (size_t)m[0], hipMemcpyDeviceToHost));
  return JDS_OK;
}

int jds_encode_jfif(jds_ctx* c, const jds_params* prm, int64_t H, int64_t W, const int16_t* coeffs, uint8_t* out,
                    int64_t out_cap, int64_t* out_len, uint64_t* scan_bits) {
  return encode_jfif(c, prm, H, W, false, coeffs, out, out_cap, out_len, scan_bits);
}

int jds_encode_jfif_rst(jds_ctx* c, const jds_params* prm, int64_t H, int64_t W, int32_t interval,
                        const int16_t* coeffs, uint8_t* out, int64_t out_cap, int64_t* out_len, uint64_t* scan_bits) {
  const int rc = check_writer_interval(interval);
  if (rc) return rc;
  return encode_jfif(c, prm, H, W, true, coeffs, out, out_cap, out_len, scan_bits);
}

// Optimised tables (DESIGN.md "Optimised tables"): interval 0 or the writer's.
static int check_opt_interval(int32_t interval) { return interval ? check_writer_interval(interval) : JDS_OK; }

int jds_plan_entropy_capacity_opt(const jds_plan* p, int32_t interval, int64_t* bytes_per_frame) {
  if (!p || !bytes_per_frame) return fail(JDS_EINVAL, "null argument");
  if (p->g.bs != 8) return fail(JDS_ENOTSUP, "JPEG entropy coding needs 8x8 blocks (block_size %d)", p->g.bs);
  const int rc = check_opt_interval(interval);
  if (rc) return rc;
  *bytes_per_frame = ent_capacity_opt(p->g, interval != 0);
  return JDS_OK;
}

int jds_plan_entropy_opt(jds_plan* p, int32_t interval, const int16_t* coeffs, uint8_t* out, int64_t out_stride,
                         uint64_t* lengths, uint64_t* scan_bits, void* stream) {
  const int rc = check_opt_interval(interval);
  if (rc) return rc;
  return plan_entropy(p, interval != 0, coeffs, out, out_stride, lengths, scan_bits, stream, true);
}

int jds_encode_jfif_opt(jds_ctx* c, const jds_params* prm, int64_t H, int64_t W, int32_t interval,
                        const int16_t* coeffs, uint8_t* out, int64_t out_cap, int64_t* out_len, uint64_t* scan_bits) {
  const int rc = check_opt_interval(interval);
  if (rc) return rc;
  return encode_jfif(c, prm, H, W, interval != 0, coeffs, out, out_cap, out_len, scan_bits, true);
}

// The fields jds_selftest_huffopt[_dev] return for a table that fell back: the Annex K AC luma table.
static void huffopt_fallback(uint8_t* bits_out, uint8_t* vals_out, int32_t* n_vals) {
  const uint8_t *b, *v;
  const int n = ent_std_table(1, &b, &v);
  memcpy(bits_out, b, 16);
  memset(vals_out, 0, 256);
  memcpy(vals_out, v, (size_t)n);
  *n_vals = n;
}

int jds_selftest_huffopt(const uint32_t* freq, uint8_t* bits_out, uint8_t* vals_out, int32_t* n_vals,
                         int32_t* fell_back) {
  if (!freq || !bits_out || !vals_out || !n_vals || !fell_back) return fail(JDS_EINVAL, "null argument");
  HoTable t;
  opt_table_host(freq, &t);
  *fell_back = t.fell_back;
  if (t.fell_back) {
    huffopt_fallback(bits_out, vals_out, n_vals);
    return JDS_OK;
  }
  memcpy(bits_out, t.bits, 16);
  memcpy(vals_out, t.vals, 256);
  *n_vals = t.n_vals;
  return JDS_OK;
}

int jds_selftest_huffopt_dev(jds_ctx* c, const uint32_t* freqs, int32_t n, uint8_t* bits_out, uint8_t* vals_out,
                             int32_t* n_vals, int32_t* fell_back) {
  if (!c || !freqs || !bits_out || !vals_out || !n_vals || !fell_back) return fail(JDS_EINVAL, "null argument");
  if (n < 1 || n > 65536) return fail(JDS_EINVAL, "n = %d histograms (1..65536)", n);
  HIP_TRY(hipSetDevice(c->device));
  hipStream_t s = c->stream;
  DevBuf d;
  const size_t o_bits = 1024 * (size_t)n, o_vals = o_bits + 16 * (size_t)n, o_nv = o_vals + 256 * (size_t)n,
               o_fell = o_nv + 4 * (size_t)n, total = o_fell + 4 * (size_t)n;
  HIP_TRY(d.ensure(total));
  char* base = (char*)d.p;
  hipError_t e = hipMemcpyAsync(base, freqs, o_bits, hipMemcpyHostToDevice, s);
  if (e == hipSuccess)
    e = launch_opt_tables_selftest(n, (const uint32_t*)base, (uint8_t*)base + o_bits, (uint8_t*)base + o_vals,
                                   (int32_t*)(base + o_nv), (int32_t*)(base + o_fell), s);
  if (e == hipSuccess) e = hipMemcpyAsync(bits_out, base + o_bits, 16 * (size_t)n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(vals_out, base + o_vals, 256 * (size_t)n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(n_vals, base + o_nv, 4 * (size_t)n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipMemcpyAsync(fell_back, base + o_fell, 4 * (size_t)n, hipMemcpyDeviceToHost, s);
  if (e == hipSuccess) e = hipStreamSynchronize(s);
  d.release();
  HIP_TRY(e);
  for (int i = 0; i < n; ++i)
    if (fell_back[i]) huffopt_fallback(bits_out + 16 * (size_t)i, vals_out + 256 * (size_t)i, n_vals + i);
  return JDS_OK;
}

// ------------------------------------------------------ entropy decoding --

int jds_jfif_parse(const uint8_t* data, int64_t len, jds_jfif_info* out) {
  const int rc = hd_parse(data, len, out, false, g_err, sizeof g_err);
  if (rc) return rc;
  if (out->H * out->W > (int64_t)1 << 28)
    return fail(JDS_EINVAL, "unsupported image size %lldx%lld", (long long)out->H, (long long)out->W);
  return JDS_OK;
}

int jds_entropy_decode_info(int32_t* subseq_bits, int32_t* subseq_per_group) {
  if (!subseq_bits || !subseq_per_group) return fail(JDS_EINVAL, "null argument");
  int s, g;
  dec_constants(&s, &g);
  *subseq_bits = s;
  *subseq_per_group = g;
  return JDS_OK;
}

int jds_selftest_huffdec(const uint8_t* data, int64_t len, int32_t subseq_bits, int16_t* coeffs, int64_t coeffs_cap,
                         int32_t* rounds_out) {
  if (!coeffs || !rounds_out) return fail(JDS_EINVAL, "null argument");
  if (subseq_bits < 64 || subseq_bits % 8) return fail(JDS_EINVAL, "subseq_bits must be a multiple of 8, at least 64");
  jds_jfif_info info;
  const int rc = jds_jfif_parse(data, len, &info);
  if (rc) return rc;
  if (coeffs_cap < info.coeffs_needed)
    return fail(JDS_EINVAL, "coefficient buffer too small: %lld entries needed", (long long)info.coeffs_needed);
  rounds_out[0] = rounds_out[1] = rounds_out[2] = 0;
  const uint32_t st = hd_host_decode(data, &info, subseq_bits, coeffs, rounds_out);
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  return JDS_OK;
}

// Where a file's descriptors point in launches that serve several files
// (jds_jpeg_batch_to_rgb); the single-file calls pass zeros.
struct FilePlace {
  int file;            // its table set (tabs + 4 * file), MCU record (mcu + file) and status word
  long long data_off;  // its first byte, from the files base
  long long coef_off;  // its first coefficient, from the coeffs base
  long long dcs_off;   // interleaved: its first entry in the DC staging array
};

// The next RSTm marker of n bytes of scan data at or after byte a (n: none).
static long long next_rst(const uint8_t* d, long long a, long long n) {
  while (a < n) {
    const uint8_t* p = (const uint8_t*)memchr(d + a, 0xFF, (size_t)(n - a));
    if (!p) break;
    const long long e = p - d;
    if (e + 1 < n && d[e + 1] >= 0xD0 && d[e + 1] <= 0xD7) return e;
    a = e + 1;
  }
  return n;
}

// Appends the descriptors and lane intervals of a parsed file with three
// non-interleaved scans.  A scan without restart intervals is one descriptor of
// the self-synchronising kernels.  With an interval of at most lane_max blocks
// every interval goes to a lane of k_dec_rst; with a larger one every interval
// is a descriptor of its own (byte range, block count, destination), whose DC
// sum is the interval's.
static int plain_descriptors(const uint8_t* data, const jds_jfif_info* info, const FilePlace& pl, int lane_max,
                             std::vector<DecScan>& sc, std::vector<RstIv>& ivs) {
  for (int i = 0; i < info->n_scans; ++i) {  // (three; one for a grayscale file)
    const jds_jfif_scan& f = info->scan[i];
    const int comp = f.component - 1;
    if (f.length >= (int64_t)1 << 40) return fail(JDS_ENOTSUP, "scan of %lld bytes", (long long)f.length);
    const long long coef_off = pl.coef_off + (comp == 0 ? 0 : 64 * (info->y_blocks + (comp - 1) * info->c_blocks));
    const long long nblocks = comp ? info->c_blocks : info->y_blocks;
    const long long ri = f.restart_interval;
    auto descriptor = [&](long long off, long long nbytes, long long blk0, long long nb) {
      DecScan d{};
      d.data_off = pl.data_off + off;
      d.nbytes = nbytes;
      d.coef_off = coef_off + 64 * blk0;
      d.nblocks = (int)nb;
      d.frame = pl.file;
      d.file = pl.file;
      d.dc_tab = 4 * pl.file + f.dc_table;
      d.ac_tab = 4 * pl.file + 2 + f.ac_table;
      sc.push_back(d);
    };
    if (ri == 0) {
      descriptor(f.offset, f.length, 0, nblocks);
      continue;
    }
    // the parser checked the markers' number and order: interval k ends at marker k
    const uint8_t* d = data + f.offset;
    long long a = 0, blk0 = 0;
    while (blk0 < nblocks) {
      const long long e = next_rst(d, a, f.length);
      const long long nb = nblocks - blk0 < ri ? nblocks - blk0 : ri;
      if (ri <= lane_max) {
        if (e - a > 0x7fffffffll) return fail(JDS_ENOTSUP, "restart interval of %lld bytes", e - a);
        RstIv v{};
        v.data_off = pl.data_off + f.offset + a;
        v.coef_off = coef_off + 64 * blk0;
        v.nbytes = (int)(e - a);
        v.nblk = (int)nb;
        v.frame = pl.file;
        v.file = pl.file;
        v.tabs = f.dc_table | ((2 + f.ac_table) << 8);
        ivs.push_back(v);
      } else {
        descriptor(f.offset + a, e - a, blk0, nb);
      }
      blk0 += nb;
      a = e + 2;
      if (e >= f.length && blk0 < nblocks) return fail(JDS_EINVAL, "restart markers missing from the scan data (DRI %lld)", ri);
    }
  }
  return JDS_OK;
}

// Upload one parsed file and decode it into c->ent_cf (device coefficients).
static int decode_file_dev(jds_ctx* c, const uint8_t* data, int64_t len, jds_jfif_info* info) {
  hipStream_t s = c->stream;
  HuffDecTab tabs[4];
  for (int i = 0; i < 4; ++i) {
    memset(&tabs[i], 0, sizeof tabs[i]);
    if (info->huff[i].defined && hd_build(info->huff[i].bits, info->huff[i].vals, &tabs[i]) < 0)
      return fail(JDS_EINVAL, "DHT: BITS over-subscribe the code space");
  }
  int lane_max;
  rst_constants(&lane_max);
  std::vector<DecScan> sc;
  std::vector<RstIv> ivs;
  int rc = plain_descriptors(data, info, FilePlace{0, 0, 0, 0}, lane_max, sc, ivs);
  if (rc) return rc;
  if (sc.size() > 0x7fffffffull) return fail(JDS_ENOTSUP, "too many restart intervals");
  const int nsc = (int)sc.size();
  int max_ngrp = 0;
  const long long ng = dec_layout(sc.data(), nsc, &max_ngrp);
  if (ng < 0) return fail(JDS_ENOTSUP, "scan too long");
  HIP_TRY(c->dec_file.ensure((size_t)len));
  HIP_TRY(c->dec_tab.ensure(sizeof tabs));
  HIP_TRY(c->dec_scr.ensure(dec_scratch_bytes(ng, nsc)));
  HIP_TRY(c->dec_st.ensure(16));
  HIP_TRY(c->dec_iv.ensure(sizeof(RstIv) * ivs.size()));
  if (!ivs.empty())
    HIP_TRY(hipMemcpyAsync(c->dec_iv.p, ivs.data(), sizeof(RstIv) * ivs.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(c->ent_cf.ensure((size_t)info->coeffs_needed * sizeof(int16_t)));
  HIP_TRY(hipMemcpyAsync(c->dec_file.p, data, (size_t)len, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->dec_tab.p, tabs, sizeof tabs, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemsetAsync(c->dec_st.p, 0, 16, s));
  HIP_TRY(hipStreamSynchronize(s));  // tabs is a stack array
  unsigned rounds = 0;
  int too_many = 0;
  // (zero-fills the coefficients; with no descriptors that is all it does, and rounds stays 0)
  HIP_TRY(dec_run((const uint8_t*)c->dec_file.p, sc.data(), nsc, ng, max_ngrp, (const HuffDecTab*)c->dec_tab.p,
                  c->dec_scr.p, (int16_t*)c->ent_cf.p, info->coeffs_needed, (uint32_t*)c->dec_st.p, s, &rounds,
                  &too_many, nullptr, nullptr));
  if (too_many) return fail(JDS_EHIP, "entropy decode: propagation did not settle within %d rounds", max_ngrp);
  HIP_TRY(launch_dec_rst((const uint8_t*)c->dec_file.p, (const RstIv*)c->dec_iv.p, (long long)ivs.size(),
                         (const HuffDecTab*)c->dec_tab.p, (int16_t*)c->ent_cf.p, (uint32_t*)c->dec_st.p, s, nullptr));
  uint32_t st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->dec_st.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  info->status = st;
  info->rounds = rounds;
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  return JDS_OK;
}

int jds_decode_jfif(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                    jds_jfif_info* info) {
  if (!c || !data || !info) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jfif_parse(data, len, info);
  if (rc) return rc;
  if (!coeffs || coeffs_cap < info->coeffs_needed)
    return fail(JDS_EINVAL, "coefficient buffer too small: %lld entries needed", (long long)info->coeffs_needed);
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_file_dev(c, data, len, info))) return rc;
  HIP_TRY(hipMemcpy(coeffs, c->ent_cf.p, (size_t)info->coeffs_needed * sizeof(int16_t), hipMemcpyDeviceToHost));
  return JDS_OK;
}

// ------------------------------------------ files of either scan form --

int jds_jpeg_parse(const uint8_t* data, int64_t len, jds_jpeg_info* out) {
  const int rc = hd_jpeg_parse(data, len, out, g_err, sizeof g_err);
  if (rc) return rc;
  if (out->H * out->W > (int64_t)1 << 28)
    return fail(JDS_EINVAL, "unsupported image size %lldx%lld", (long long)out->H, (long long)out->W);
  return JDS_OK;
}

int jds_selftest_jpegdec(const uint8_t* data, int64_t len, int32_t subseq_bits, int16_t* coeffs, int64_t coeffs_cap,
                         int32_t* rounds_out) {
  if (!coeffs || !rounds_out) return fail(JDS_EINVAL, "null argument");
  if (subseq_bits < 64 || subseq_bits % 8) return fail(JDS_EINVAL, "subseq_bits must be a multiple of 8, at least 64");
  jds_jpeg_info info;
  const int rc = jds_jpeg_parse(data, len, &info);
  if (rc) return rc;
  if (coeffs_cap < info.coeffs_needed)
    return fail(JDS_EINVAL, "coefficient buffer too small: %lld entries needed", (long long)info.coeffs_needed);
  int lane_max;
  rst_constants(&lane_max);
  const uint32_t st = hd_jpeg_host_decode(data, &info, subseq_bits, lane_max, coeffs, rounds_out);
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  return JDS_OK;
}

// Appends the descriptors and lane intervals of a parsed file with one
// interleaved scan (m: its MCU record, whose off[] hold the file's place in the
// coefficient buffer).  Routing as plain_descriptors': no restart interval ->
// one descriptor; intervals of at most lane_max blocks (Ri * blocks per MCU) ->
// one lane of k_dec_rst each; longer ones -> one descriptor each.
static int il_descriptors(const uint8_t* data, const jds_jpeg_info* info, const HdMcu& m, const FilePlace& pl,
                          int lane_max, std::vector<DecScan>& sc, std::vector<RstIv>& ivs) {
  const jds_jpeg_scan& f = info->scan[0];
  if (f.length >= (int64_t)1 << 40) return fail(JDS_ENOTSUP, "scan of %lld bytes", (long long)f.length);
  const long long nblocks = (long long)m.bpm * m.mcu_cols * m.mcu_rows;
  if (nblocks > 0x7fffffffll) return fail(JDS_ENOTSUP, "scan of %lld blocks", nblocks);
  const long long rib = (long long)f.restart_interval * m.bpm;
  auto descriptor = [&](long long off, long long nbytes, long long blk0, long long nb) {
    DecScan d{};
    d.data_off = pl.data_off + off;
    d.nbytes = nbytes;
    d.coef_off = 0;
    d.dcs_off = pl.dcs_off;
    d.nblocks = (int)nb;
    d.frame = pl.file;
    d.file = pl.file;
    d.blk_base = (int)blk0;
    sc.push_back(d);
  };
  if (rib == 0) {
    descriptor(f.offset, f.length, 0, nblocks);
    return JDS_OK;
  }
  const uint8_t* d = data + f.offset;
  long long a = 0, blk0 = 0;
  while (blk0 < nblocks) {
    const long long e = next_rst(d, a, f.length);
    const long long nb = nblocks - blk0 < rib ? nblocks - blk0 : rib;
    if (rib <= lane_max) {
      if (e - a > 0x7fffffffll) return fail(JDS_ENOTSUP, "restart interval of %lld bytes", e - a);
      RstIv v{};
      v.data_off = pl.data_off + f.offset + a;
      v.coef_off = blk0;
      v.nbytes = (int)(e - a);
      v.nblk = (int)nb;
      v.frame = pl.file;
      v.file = pl.file;
      ivs.push_back(v);
    } else {
      descriptor(f.offset + a, e - a, blk0, nb);
    }
    blk0 += nb;
    a = e + 2;
    if (e >= f.length && blk0 < nblocks)
      return fail(JDS_EINVAL, "restart markers missing from the scan data (DRI %d)", f.restart_interval);
  }
  return JDS_OK;
}

// Upload a parsed file with one interleaved scan and decode it into c->ent_cf.
static int decode_il_dev(jds_ctx* c, const uint8_t* data, int64_t len, jds_jpeg_info* info) {
  hipStream_t s = c->stream;
  HuffDecTab tabs[4];
  for (int i = 0; i < 4; ++i) {
    memset(&tabs[i], 0, sizeof tabs[i]);
    if (info->huff[i].defined && hd_build(info->huff[i].bits, info->huff[i].vals, &tabs[i]) < 0)
      return fail(JDS_EINVAL, "DHT: BITS over-subscribe the code space");
  }
  const HdMcu m = hd_jpeg_mcu(info);
  const long long nblocks = (long long)m.bpm * m.mcu_cols * m.mcu_rows;
  int lane_max;
  rst_constants(&lane_max);
  std::vector<DecScan> sc;
  std::vector<RstIv> ivs;
  int rc = il_descriptors(data, info, m, FilePlace{0, 0, 0, 0}, lane_max, sc, ivs);
  if (rc) return rc;
  if (sc.size() > 0x7fffffffull) return fail(JDS_ENOTSUP, "too many restart intervals");
  const int nsc = (int)sc.size();
  int max_ngrp = 0;
  const long long ng = dec_layout(sc.data(), nsc, &max_ngrp);
  if (ng < 0) return fail(JDS_ENOTSUP, "scan too long");
  const size_t dcs_off = (sizeof(HdMcu) + 15) & ~(size_t)15;
  HIP_TRY(c->dec_file.ensure((size_t)len));
  HIP_TRY(c->dec_tab.ensure(sizeof tabs));
  HIP_TRY(c->dec_scr.ensure(dec_scratch_bytes(ng, nsc)));
  HIP_TRY(c->dec_st.ensure(16));
  HIP_TRY(c->dec_iv.ensure(sizeof(RstIv) * ivs.size()));
  HIP_TRY(c->dec_mcu.ensure(dcs_off + sizeof(int16_t) * (size_t)nblocks));
  if (!ivs.empty())
    HIP_TRY(hipMemcpyAsync(c->dec_iv.p, ivs.data(), sizeof(RstIv) * ivs.size(), hipMemcpyHostToDevice, s));
  HIP_TRY(c->ent_cf.ensure((size_t)info->coeffs_needed * sizeof(int16_t)));
  HIP_TRY(hipMemcpyAsync(c->dec_file.p, data, (size_t)len, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->dec_tab.p, tabs, sizeof tabs, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(c->dec_mcu.p, &m, sizeof m, hipMemcpyHostToDevice, s));
  int16_t* dcs = (int16_t*)((char*)c->dec_mcu.p + dcs_off);
  HIP_TRY(hipMemsetAsync(dcs, 0, sizeof(int16_t) * (size_t)nblocks, s));
  HIP_TRY(hipMemsetAsync(c->dec_st.p, 0, 16, s));
  HIP_TRY(hipStreamSynchronize(s));  // tabs and m are stack objects
  unsigned rounds = 0;
  int too_many = 0;
  HIP_TRY(dec_run((const uint8_t*)c->dec_file.p, sc.data(), nsc, ng, max_ngrp, (const HuffDecTab*)c->dec_tab.p,
                  c->dec_scr.p, (int16_t*)c->ent_cf.p, info->coeffs_needed, (uint32_t*)c->dec_st.p, s, &rounds,
                  &too_many, (const HdMcu*)c->dec_mcu.p, dcs));
  if (too_many) return fail(JDS_EHIP, "entropy decode: propagation did not settle within %d rounds", max_ngrp);
  HIP_TRY(launch_dec_rst((const uint8_t*)c->dec_file.p, (const RstIv*)c->dec_iv.p, (long long)ivs.size(),
                         (const HuffDecTab*)c->dec_tab.p, (int16_t*)c->ent_cf.p, (uint32_t*)c->dec_st.p, s,
                         (const HdMcu*)c->dec_mcu.p));
  uint32_t st = 0;
  HIP_TRY(hipMemcpyAsync(&st, c->dec_st.p, 4, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  info->status = st;
  info->rounds = rounds;
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  return JDS_OK;
}

// A file of three non-interleaved scans (a grayscale file: of one) in the terms
// of the first decoder.
static void jfif_view(const jds_jpeg_info* info, jds_jfif_info* fi) {
  memset(fi, 0, sizeof *fi);
  fi->H = info->H;
  fi->W = info->W;
  fi->subsampling = info->subsampling;
  fi->n_scans = info->n_scans;
  for (int i = 0; i < info->n_scans; ++i) {
    const jds_jpeg_scan& f = info->scan[i];
    fi->scan[i].component = f.component[0];
    fi->scan[i].dc_table = f.dc_table[0];
    fi->scan[i].ac_table = f.ac_table[0];
    fi->scan[i].restart_interval = f.restart_interval;
    fi->scan[i].offset = f.offset;
    fi->scan[i].length = f.length;
  }
  memcpy(fi->huff, info->huff, sizeof fi->huff);
  fi->y_blocks = info->grid_cols[0] * info->grid_rows[0];
  fi->c_blocks = info->grid_cols[1] * info->grid_rows[1];
  fi->coeffs_needed = info->coeffs_needed;
}

// A parsed file of either scan form into c->ent_cf.
static int decode_jpeg_dev(jds_ctx* c, const uint8_t* data, int64_t len, jds_jpeg_info* info) {
  int rc;
  if (info->interleaved) {
    rc = decode_il_dev(c, data, len, info);
  } else {
    // three non-interleaved scans: the existing route, over the T.81 grids (a
    // non-interleaved scan holds exactly its component's grid, T.81 A.2.2)
    jds_jfif_info fi;
    jfif_view(info, &fi);
    rc = decode_file_dev(c, data, len, &fi);
    info->status = fi.status;
    info->rounds = fi.rounds;
  }
  return rc;
}

int jds_decode_jpeg(jds_ctx* c, const uint8_t* data, int64_t len, int16_t* coeffs, int64_t coeffs_cap,
                    jds_jpeg_info* info) {
  if (!c || !data || !info) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  if (!coeffs || coeffs_cap < info->coeffs_needed)
    return fail(JDS_EINVAL, "coefficient buffer too small: %lld entries needed", (long long)info->coeffs_needed);
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_jpeg_dev(c, data, len, info))) return rc;
  HIP_TRY(hipMemcpy(coeffs, c->ent_cf.p, (size_t)info->coeffs_needed * sizeof(int16_t), hipMemcpyDeviceToHost));
  return JDS_OK;
}

static int inverse_of_decoded(jds_ctx* c, const jds_params* prm, int64_t H, int64_t W, int64_t n_coeffs,
                              uint8_t* rgb_out, int16_t* coeffs);

int jds_decompress_jpeg(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                        int16_t* coeffs, jds_jpeg_info* info) {
  if (!c || !data || !info || !rgb_out) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  if (info->subsampling == JDS_SS_GRAY)
    return fail(JDS_ENOTSUP, "the plan's inverse takes three components: this is a grayscale file "
                             "(jds_jpeg_to_rgb reconstructs it)");
  if (!info->single_table || !info->reference_grid)
    return fail(JDS_ENOTSUP, "the plan's inverse takes one quantisation table and the reference's block grids: "
                             "%s (the per-stage calls reconstruct such a file)",
                info->single_table ? "this size has other grids" : "the file has a table per component");
  const size_t nimg = (size_t)info->H * (size_t)info->W * 3;
  if (rgb_cap < (int64_t)nimg) return fail(JDS_EINVAL, "image buffer too small: %zu bytes needed", nimg);
  jds_params prm;
  memset(&prm, 0, sizeof prm);
  prm.block_size = 8;
  prm.quality = 0;
  prm.subsampling = info->subsampling;
  memcpy(prm.qtable, info->qtable[0], sizeof prm.qtable);
  if ((rc = check_tables(&prm))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_jpeg_dev(c, data, len, info))) return rc;
  return inverse_of_decoded(c, &prm, info->H, info->W, info->coeffs_needed, rgb_out, coeffs);
}

// ----------------------------------- foreign files to pixels (k_jpeg_inv) --

int jds_jpeg_inverse_info(int32_t* tile_h, int32_t* tile_w) {
  if (!tile_h || !tile_w) return fail(JDS_EINVAL, "null argument");
  int th, tw;
  jpeg_inv_constants(&th, &tw);
  *tile_h = th;
  *tile_w = tw;
  return JDS_OK;
}

// The rendering a _render call names: JDS_RENDER_REFERENCE (k_jpeg_inv) or
// JDS_RENDER_LIBJPEG (k_jpeg_ljt); anything else is the caller's error.
static int render_check(int32_t render) {
  if (render != JDS_RENDER_REFERENCE && render != JDS_RENDER_LIBJPEG)
    return fail(JDS_EINVAL, "unknown render %d (JDS_RENDER_REFERENCE or JDS_RENDER_LIBJPEG)", (int)render);
  return JDS_OK;
}

// The launch arguments of a parsed file: its tables by check_tables' rule, its
// grids T.81's for H x W, every tile's chroma window within the kernel's arrays.
static int jpeg_inv_args(const jds_jpeg_info* info, JInvArgs* a) {
  const int rc = jinv_args(info, a);
  if (rc == -1000)
    return fail(JDS_EINVAL, "jpeg inverse: %lldx%lld with these grids is not a T.81 geometry of subsampling %d",
                (long long)info->H, (long long)info->W, info->subsampling);
  if (rc < 0) {
    const int c = (-rc - 1) / 64, i = (-rc - 1) % 64;
    return fail(JDS_EINVAL, "qtable[%d][%d] = %g is not an integer in [1, 255]", c, i, info->qtable[c][i]);
  }
  if (!jpeg_inv_fits(*a))
    return fail(JDS_ENOTSUP, "jpeg inverse: a tile of %lldx%lld reads a wider chroma window than the kernel keeps",
                (long long)info->H, (long long)info->W);
  return JDS_OK;
}

static hipError_t launch_render(int32_t render, const JInvArgs& a, const int16_t* coeffs, uint8_t* rgb, hipStream_t s) {
  return render == JDS_RENDER_LIBJPEG ? launch_jpeg_ljt(a, coeffs, rgb, s) : launch_jpeg_inv(a, coeffs, rgb, s);
}

int jds_jpeg_render_dev(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb, void* stream,
                        int32_t render) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!info) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  if (!c || !coeffs || !rgb) return fail(JDS_EINVAL, "null argument");
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(launch_render(render, a, coeffs, rgb, (hipStream_t)stream));
  return JDS_OK;
}

int jds_jpeg_inverse_dev(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb, void* stream) {
  return jds_jpeg_render_dev(c, info, coeffs, rgb, stream, JDS_RENDER_REFERENCE);
}

int jds_jpeg_to_rgb(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                    int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info) {
  return jds_jpeg_to_rgb_render(c, data, len, rgb_out, rgb_cap, rgb_on_device, coeffs, info, JDS_RENDER_REFERENCE);
}

int jds_jpeg_to_rgb_render(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                           int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_info* info, int32_t render) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!c || !data || !info || !rgb_out) return fail(JDS_EINVAL, "null argument");
  rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  const size_t nimg = (size_t)info->H * (size_t)info->W * 3;
  if (rgb_cap < (int64_t)nimg) return fail(JDS_EINVAL, "image buffer too small: %zu bytes needed", nimg);
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_jpeg_dev(c, data, len, info))) return rc;  // (a defective scan: rgb_out is not written)
  uint8_t* dst = rgb_out;
  if (!rgb_on_device) {
    HIP_TRY(c->out.ensure(nimg));
    dst = (uint8_t*)c->out.p;
  }
  HIP_TRY(launch_render(render, a, (const int16_t*)c->ent_cf.p, dst, c->stream));
  if (!rgb_on_device) HIP_TRY(hipMemcpyAsync(rgb_out, dst, nimg, hipMemcpyDeviceToHost, c->stream));
  if (coeffs)
    HIP_TRY(hipMemcpyAsync(coeffs, c->ent_cf.p, (size_t)info->coeffs_needed * sizeof(int16_t), hipMemcpyDeviceToHost,
                           c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return JDS_OK;
}

int jds_selftest_jpeg_render(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out, int32_t render) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!info || !coeffs || !rgb_out) return fail(JDS_EINVAL, "null argument");
  JInvArgs a;
  if ((rc = jpeg_inv_args(info, &a))) return rc;
  if (render == JDS_RENDER_LIBJPEG)
    jpeg_ljt_host_image(a, coeffs, rgb_out);
  else
    jpeg_inv_host(a, coeffs, rgb_out);
  return JDS_OK;
}

int jds_selftest_jpeg_inverse(const jds_jpeg_info* info, const int16_t* coeffs, uint8_t* rgb_out) {
  return jds_selftest_jpeg_render(info, coeffs, rgb_out, JDS_RENDER_REFERENCE);
}

int jds_selftest_jpeg_window(int32_t d0, int32_t d1, int32_t dst_n, int32_t src_n, int32_t xaxis, int32_t* out) {
  if (!out || dst_n < 1 || src_n < 1 || d0 < 0 || d1 < d0 || d1 >= dst_n) return fail(JDS_EINVAL, "bad argument");
  jpeg_inv_window(d0, d1, 1.0 / ((double)dst_n / (double)src_n), src_n, xaxis != 0, &out[0], &out[1]);
  out[2] = JI_CAP_ROWS2;
  out[3] = JI_CAP_COLS2;
  return JDS_OK;
}

// ------------------------------------------- batches of foreign files --
// (DESIGN.md "Batches of foreign files")

// What the layout keeps per batch: the parsed files, the inverse records of the
// ones that take part (in batch order) and the tile maps of the four launches.
struct BatchPlan {
  std::vector<jds_jpeg_info> info;  // per file
  std::vector<int> rec_of;          // per file: its record, or -1
  std::vector<int> file_of;         // per record: its file
  std::vector<JInvRec> recs;
  std::vector<JInvMap> map[JI_MODES];
  int64_t rgb_bytes = 0, coef_entries = 0;
  int first_bad = -1;
  char first_msg[400] = "";
};

// Parse every file, check what the single call checks before it decodes, and
// lay the outputs out: images JI_RGB_ALIGN apart at least, coefficients end to
// end.  A file that fails takes no space and does not stop the batch.
static int batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items,
                        BatchPlan& bp) {
  if (n < 0 || (n > 0 && (!data || !lens || !items))) return fail(JDS_EINVAL, "null argument");
  bp.info.resize((size_t)n);
  bp.rec_of.assign((size_t)n, -1);
  std::vector<JInvRec> parsed((size_t)n);
  std::vector<std::string> msg((size_t)n);  // (the message of a failing file: g_err is per thread)
  batch_parallel(n, [&](int i) {
    jds_jpeg_batch_item& it = items[i];
    memset(&it, 0, sizeof it);
    it.rgb_off = -1;
    it.coef_off = -1;
    jds_jpeg_info& info = bp.info[(size_t)i];
    JInvRec& r = parsed[(size_t)i];
    memset(&r, 0, sizeof r);
    int rc = data[i] && lens[i] >= 0 ? jds_jpeg_parse(data[i], lens[i], &info) : fail(JDS_EINVAL, "null file");
    if (rc == JDS_OK) {
      it.H = info.H;
      it.W = info.W;
      it.subsampling = info.subsampling;
      it.interleaved = info.interleaved;
      rc = jpeg_inv_args(&info, &r.a);
    }
    if (rc == JDS_OK) {
      HuffDecTab t;
      for (int k = 0; k < 4 && rc == JDS_OK; ++k)
        if (info.huff[k].defined && hd_build(info.huff[k].bits, info.huff[k].vals, &t) < 0)
          rc = fail(JDS_EINVAL, "DHT: BITS over-subscribe the code space");
    }
    it.rc = rc;
    if (rc != JDS_OK) msg[(size_t)i] = g_err;
  });
  for (int i = 0; i < n; ++i) {
    jds_jpeg_batch_item& it = items[i];
    const jds_jpeg_info& info = bp.info[(size_t)i];
    JInvRec& r = parsed[(size_t)i];
    if (it.rc != JDS_OK) {
      if (bp.first_bad < 0) {
        bp.first_bad = i;
        snprintf(bp.first_msg, sizeof bp.first_msg, "%s", msg[(size_t)i].c_str());
      }
      continue;
    }
    long long rb = bp.rgb_bytes, ce = bp.coef_entries;
    jinv_batch_place(r, (int)bp.recs.size(), info.coeffs_needed, &rb, &ce);
    bp.rgb_bytes = rb;
    bp.coef_entries = ce;
    it.rgb_off = r.rgb_off;
    it.coef_off = r.coef_off;
    it.coeffs_needed = info.coeffs_needed;
    bp.rec_of[(size_t)i] = r.st;
    bp.file_of.push_back(i);
    bp.recs.push_back(r);
  }
  // what the grids and the 32-bit indices of the kernels take
  if (bp.coef_entries / 64 > 0x7fffffffll || !jinv_batch_maps(bp.recs.data(), (int)bp.recs.size(), bp.map))
    return fail(JDS_ENOTSUP, "batch of %d files: too many blocks or tiles for one set of launches", n);
  return JDS_OK;
}

// The first failing file by index, where jds_last_error finds it.
static void batch_note(const BatchPlan& bp) {
  if (bp.first_bad >= 0) {
    char m[400];
    snprintf(m, sizeof m, "%s", bp.first_msg);
    fail(0, "file %d: %s", bp.first_bad, m);
  } else {
    g_err[0] = 0;
  }
}

int jds_jpeg_batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items,
                          int64_t* rgb_bytes, int64_t* coef_entries) {
  if (!rgb_bytes || !coef_entries) return fail(JDS_EINVAL, "null argument");
  BatchPlan bp;
  const int rc = batch_layout(data, lens, n, items, bp);
  if (rc) return rc;
  *rgb_bytes = bp.rgb_bytes;
  *coef_entries = bp.coef_entries;
  batch_note(bp);
  return JDS_OK;
}

int jds_selftest_jpeg_batch(const uint8_t* const* data, const int64_t* lens, int32_t n, int32_t subseq_bits,
                            uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs, jds_jpeg_batch_item* items) {
  return jds_selftest_jpeg_batch_render(data, lens, n, subseq_bits, rgb, rgb_cap, coeffs, items, JDS_RENDER_REFERENCE);
}

int jds_selftest_jpeg_batch_render(const uint8_t* const* data, const int64_t* lens, int32_t n, int32_t subseq_bits,
                                   uint8_t* rgb, int64_t rgb_cap, int16_t* coeffs, jds_jpeg_batch_item* items,
                                   int32_t render) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (subseq_bits < 64 || subseq_bits % 8) return fail(JDS_EINVAL, "subseq_bits must be a multiple of 8, at least 64");
  BatchPlan bp;
  rc = batch_layout(data, lens, n, items, bp);
  if (rc) return rc;
  if (bp.rgb_bytes > 0 && (!rgb || rgb_cap < bp.rgb_bytes))
    return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", (long long)bp.rgb_bytes);
  std::vector<int16_t> own;
  if (!coeffs) {
    own.resize((size_t)bp.coef_entries);
    coeffs = own.data();
  }
  int lane_max;
  rst_constants(&lane_max);
  std::vector<uint32_t> st(bp.recs.size() + 1, 0u);
  for (size_t k = 0; k < bp.recs.size(); ++k) {
    const int i = bp.file_of[k];
    int32_t rounds[3];
    st[k] = hd_jpeg_host_decode(data[i], &bp.info[(size_t)i], subseq_bits, lane_max, coeffs + bp.recs[k].coef_off, rounds);
    items[i].status = st[k];
  }
  const JInvMap* maps[JI_MODES];
  int nmap[JI_MODES];
  for (int m = 0; m < JI_MODES; ++m) {
    maps[m] = bp.map[m].data();
    nmap[m] = (int)bp.map[m].size() - 1;
  }
  if (render == JDS_RENDER_LIBJPEG)
    jpeg_ljt_batch_host(bp.recs.data(), maps, nmap, st.data(), coeffs, rgb);
  else
    jpeg_inv_batch_host(bp.recs.data(), maps, nmap, st.data(), coeffs, rgb);
  batch_note(bp);
  return JDS_OK;
}

// The launches of a laid-out batch with at least one record: upload, entropy
// decode into c->ent_cf (file k's coefficients at bp.recs[k].coef_off), then
// with `inverse` the batch inverse into rgb; the status words into items.
// Synchronous.  Without `inverse` (jds_jpeg_batch_transcode) rgb is not used.
static int batch_run(jds_ctx* c, BatchPlan& bp, const uint8_t* const* data, const int64_t* lens, uint8_t* rgb,
                     int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items, uint32_t* rounds_out,
                     bool inverse, int32_t render = JDS_RENDER_REFERENCE) {
  int rc;
  const int nv = (int)bp.recs.size();
  hipStream_t s = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  int lane_max;
  rst_constants(&lane_max);
  const int rst_g = rst_group_lanes();
  // the upload: every part at a 256-byte boundary, files at 16-byte ones inside theirs
  auto up = [](size_t v, size_t a) { return (v + a - 1) / a * a; };
  std::vector<size_t> foff((size_t)nv);
  size_t o = 0;
  for (int k = 0; k < nv; ++k) {
    foff[(size_t)k] = o;
    o = up(o + (size_t)lens[bp.file_of[(size_t)k]], 16);
  }
  // descriptors of both decode groups, lane intervals of both forms (a file's padded to whole workgroups)
  std::vector<DecScan> sc_il, sc_pl;
  std::vector<RstIv> iv_il, iv_pl;
  std::vector<HuffDecTab> tabs(4 * (size_t)nv);
  std::vector<HdMcu> mcus((size_t)nv);
  std::vector<uint32_t> st0((size_t)nv, 0u);
  long long dcs_n = 0;
  for (int k = 0; k < nv; ++k) {
    const int i = bp.file_of[(size_t)k];
    const jds_jpeg_info& info = bp.info[(size_t)i];
    for (int t = 0; t < 4; ++t) {
      memset(&tabs[4 * (size_t)k + t], 0, sizeof(HuffDecTab));
      if (info.huff[t].defined) (void)hd_build(info.huff[t].bits, info.huff[t].vals, &tabs[4 * (size_t)k + t]);
    }
    memset(&mcus[(size_t)k], 0, sizeof(HdMcu));
    const FilePlace pl{k, (long long)foff[(size_t)k], bp.recs[(size_t)k].coef_off, dcs_n};
    std::vector<DecScan>& sc = info.interleaved ? sc_il : sc_pl;
    std::vector<RstIv>& iv = info.interleaved ? iv_il : iv_pl;
    const size_t nsc0 = sc.size(), niv0 = iv.size();
    if (info.interleaved) {
      HdMcu m = hd_jpeg_mcu(&info);
      for (int cc = 0; cc < 3; ++cc) m.off[cc] += pl.coef_off;
      mcus[(size_t)k] = m;
      rc = il_descriptors(data[i], &info, m, pl, lane_max, sc, iv);
      dcs_n += (long long)m.bpm * m.mcu_cols * m.mcu_rows;
    } else {
      jds_jfif_info fi;
      jfif_view(&info, &fi);
      rc = plain_descriptors(data[i], &fi, pl, lane_max, sc, iv);
    }
    if (rc == JDS_EINVAL) {  // restart markers missing from the scan data: a defective scan, nothing of it is decoded
      sc.resize(nsc0);
      iv.resize(niv0);
      st0[(size_t)k] = HD_RESTART;
      rc = JDS_OK;
    }
    if (rc) return rc;
    while (iv.size() % (size_t)rst_g) {
      RstIv v{};
      v.file = v.frame = k;
      iv.push_back(v);
    }
  }
  if (sc_il.size() > 0x7fffffffull || sc_pl.size() > 0x7fffffffull || iv_il.size() > 0x7fffffffull ||
      iv_pl.size() > 0x7fffffffull)
    return fail(JDS_ENOTSUP, "too many restart intervals");
  int mx_il = 0, mx_pl = 0;
  const long long ng_il = dec_layout(sc_il.data(), (int)sc_il.size(), &mx_il);
  const long long ng_pl = dec_layout(sc_pl.data(), (int)sc_pl.size(), &mx_pl);
  if (ng_il < 0 || ng_pl < 0) return fail(JDS_ENOTSUP, "batch too long for one decode");
  int map_off[JI_MODES], nmap[JI_MODES], tiles[JI_MODES], nm = 0;
  for (int m = 0; m < JI_MODES; ++m) {
    map_off[m] = nm;
    nmap[m] = (int)bp.map[m].size() - 1;
    tiles[m] = bp.map[m].back().tile0;
    nm += (int)bp.map[m].size();
  }
  const size_t o_files = 0, o_tabs = up(o, 256), o_mcu = up(o_tabs + sizeof(HuffDecTab) * tabs.size(), 256),
               o_rec = up(o_mcu + sizeof(HdMcu) * mcus.size(), 256), o_map = up(o_rec + sizeof(JInvRec) * (size_t)nv, 256),
               o_ivil = up(o_map + sizeof(JInvMap) * (size_t)nm, 256), o_ivpl = up(o_ivil + sizeof(RstIv) * iv_il.size(), 256),
               o_st = up(o_ivpl + sizeof(RstIv) * iv_pl.size(), 256), total = up(o_st + 4 * (size_t)nv, 256);
  if (total > c->bat_host_cap) {
    if (c->bat_host) (void)hipHostFree(c->bat_host);
    c->bat_host = nullptr;
    c->bat_host_cap = 0;
    HIP_TRY(hipHostMalloc(&c->bat_host, total, hipHostMallocDefault));
    c->bat_host_cap = total;
  }
  char* h = (char*)c->bat_host;
  batch_parallel(nv, [&](int k) {
    const int i = bp.file_of[(size_t)k];
    memcpy(h + o_files + foff[(size_t)k], data[i], (size_t)lens[i]);
  });
  memcpy(h + o_tabs, tabs.data(), sizeof(HuffDecTab) * tabs.size());
  memcpy(h + o_mcu, mcus.data(), sizeof(HdMcu) * mcus.size());
  memcpy(h + o_rec, bp.recs.data(), sizeof(JInvRec) * (size_t)nv);
  for (int m = 0; m < JI_MODES; ++m)
    memcpy(h + o_map + sizeof(JInvMap) * (size_t)map_off[m], bp.map[m].data(), sizeof(JInvMap) * bp.map[m].size());
  if (!iv_il.empty()) memcpy(h + o_ivil, iv_il.data(), sizeof(RstIv) * iv_il.size());
  if (!iv_pl.empty()) memcpy(h + o_ivpl, iv_pl.data(), sizeof(RstIv) * iv_pl.size());
  memcpy(h + o_st, st0.data(), 4 * (size_t)nv);
  const size_t scr_il = (dec_scratch_bytes(ng_il, (int)sc_il.size()) + 255) & ~(size_t)255;
  HIP_TRY(c->bat.ensure(total));
  HIP_TRY(c->dec_scr.ensure(scr_il + dec_scratch_bytes(ng_pl, (int)sc_pl.size())));
  HIP_TRY(c->dec_mcu.ensure(sizeof(int16_t) * (size_t)dcs_n));
  HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)bp.coef_entries));
  uint8_t* dst = rgb;
  if (inverse && !rgb_on_device) {
    HIP_TRY(c->out.ensure((size_t)bp.rgb_bytes));
    dst = (uint8_t*)c->out.p;
  }
  char* dv = (char*)c->bat.p;
  const CtxMarkScope marks_(c, s);
  HIP_TRY(hipMemcpyAsync(dv, h, total, hipMemcpyHostToDevice, s));
  if (dcs_n) HIP_TRY(hipMemsetAsync(c->dec_mcu.p, 0, sizeof(int16_t) * (size_t)dcs_n, s));
  kmark(s, "(batch upload)");
  const uint8_t* files_d = (const uint8_t*)(dv + o_files);
  const HuffDecTab* tabs_d = (const HuffDecTab*)(dv + o_tabs);
  const HdMcu* mcu_d = (const HdMcu*)(dv + o_mcu);
  uint32_t* st_d = (uint32_t*)(dv + o_st);
  int16_t* cf_d = (int16_t*)c->ent_cf.p;
  const DecGroup grp[2] = {{sc_il.data(), (int)sc_il.size(), ng_il, mx_il, c->dec_scr.p, true},
                           {sc_pl.data(), (int)sc_pl.size(), ng_pl, mx_pl, (char*)c->dec_scr.p + scr_il, false}};
  unsigned rounds = 0;
  int too_many = 0;
  HIP_TRY(dec_run_groups(files_d, grp, 2, tabs_d, cf_d, bp.coef_entries, st_d, s, &rounds, &too_many, mcu_d,
                         (int16_t*)c->dec_mcu.p));
  if (too_many)
    return fail(JDS_EHIP, "entropy decode: propagation did not settle within %d rounds", mx_il > mx_pl ? mx_il : mx_pl);
  HIP_TRY(launch_dec_rst(files_d, (const RstIv*)(dv + o_ivil), (long long)iv_il.size(), tabs_d, cf_d, st_d, s, mcu_d));
  HIP_TRY(launch_dec_rst(files_d, (const RstIv*)(dv + o_ivpl), (long long)iv_pl.size(), tabs_d, cf_d, st_d, s, nullptr));
  if (inverse && render == JDS_RENDER_LIBJPEG)
    HIP_TRY(launch_jpeg_ljt_batch((const JInvRec*)(dv + o_rec), (const JInvMap*)(dv + o_map), map_off, nmap, tiles,
                                  st_d, cf_d, dst, s));
  else if (inverse)
    HIP_TRY(launch_jpeg_inv_batch((const JInvRec*)(dv + o_rec), (const JInvMap*)(dv + o_map), map_off, nmap, tiles,
                                  st_d, cf_d, dst, s));
  if (inverse && !rgb_on_device)  // image by image: the gaps of the caller's buffer stay as they are
    for (int k = 0; k < nv; ++k) {
      const JInvRec& r = bp.recs[(size_t)k];
      HIP_TRY(hipMemcpyAsync(rgb + r.rgb_off, dst + r.rgb_off, (size_t)r.a.H * (size_t)r.a.W * 3, hipMemcpyDeviceToHost,
                             s));
    }
  if (coeffs)
    HIP_TRY(hipMemcpyAsync(coeffs, cf_d, sizeof(int16_t) * (size_t)bp.coef_entries, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(st0.data(), st_d, 4 * (size_t)nv, hipMemcpyDeviceToHost, s));
  kmark(s, "(batch download)");
  HIP_TRY(hipStreamSynchronize(s));
  for (int k = 0; k < nv; ++k) items[bp.file_of[(size_t)k]].status = st0[(size_t)k];
  if (rounds_out) *rounds_out = rounds;
  return JDS_OK;
}

int jds_jpeg_batch_to_rgb(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                          int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items,
                          uint32_t* rounds_out) {
  return jds_jpeg_batch_to_rgb_render(c, data, lens, n, rgb, rgb_cap, rgb_on_device, coeffs, items, rounds_out,
                                      JDS_RENDER_REFERENCE);
}

int jds_jpeg_batch_to_rgb_render(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, uint8_t* rgb,
                                 int64_t rgb_cap, int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items,
                                 uint32_t* rounds_out, int32_t render) {
  int rc;
  if ((rc = render_check(render))) return rc;
  if (!c) return fail(JDS_EINVAL, "null argument");
  BatchPlan bp;
  rc = batch_layout(data, lens, n, items, bp);
  if (rc) return rc;
  if (rounds_out) *rounds_out = 0;
  if (bp.rgb_bytes > 0 && (!rgb || rgb_cap < bp.rgb_bytes))
    return fail(JDS_EINVAL, "image buffer too small: %lld bytes needed", (long long)bp.rgb_bytes);
  if (!bp.recs.empty() &&
      (rc = batch_run(c, bp, data, lens, rgb, rgb_on_device, coeffs, items, rounds_out, true, render)))
    return rc;
  batch_note(bp);
  return JDS_OK;
}

// ------------------------------------------------- lossless transcode --
// (DESIGN.md "Transcode"; kernels: jds_entropy_mcu.hip)

// One file of a writer batch: its geometry record (the planes' offsets count
// from the start of c->ent_cf) and its header prefix.
struct McuJob {
  McuFile f;
  std::vector<uint8_t> pfx;
};

static int mcu_job_geo(const jds_jpeg_info* info, int64_t coef_off, McuJob* j) {
  if (mcu_file_of(info, &j->f))
    return fail(JDS_EINVAL,
                "%lldx%lld with block grids %lldx%lld, %lldx%lld, %lldx%lld is not a T.81 geometry of subsampling %d",
                (long long)info->H, (long long)info->W, (long long)info->grid_rows[0], (long long)info->grid_cols[0],
                (long long)info->grid_rows[1], (long long)info->grid_cols[1], (long long)info->grid_rows[2],
                (long long)info->grid_cols[2], info->subsampling);
  for (int cc = 0; cc < 3; ++cc) j->f.off[cc] += coef_off;
  return JDS_OK;
}

static int mcu_job_splice(const uint8_t* data, int64_t len, McuJob* j) {
  const int64_t n = mcu_splice(data, len, nullptr, 0);
  if (n < 0 || n > 0x7fffffffll) return fail(JDS_EINVAL, "header splice: no marker sequence from SOI to an SOS");
  j->pfx.resize((size_t)n);
  if (mcu_splice(data, len, j->pfx.data(), n) != n) return fail(JDS_EINVAL, "header splice: length mismatch");
  return JDS_OK;
}

static int mcu_job_prefix(const jds_jpeg_info* info, const uint8_t* prefix, int64_t prefix_len, McuJob* j) {
  if (prefix) {
    if (prefix_len < 0 || prefix_len > 0x7fffffffll) return fail(JDS_EINVAL, "prefix_len %lld", (long long)prefix_len);
    j->pfx.assign(prefix, prefix + prefix_len);
    return JDS_OK;
  }
  j->pfx.resize(MCU_PFX_DEFAULT_MAX);
  const int n = mcu_default_prefix(info, j->pfx.data());
  if (n == -1000) return fail(JDS_EINVAL, "quantisation table id outside 0..3");
  if (n < 0) {
    const int cc = (-n - 1) / 64, i = (-n - 1) % 64;
    return fail(JDS_EINVAL, "qtable[%d][%d] = %g is not an integer in [1, 255]", cc, i, info->qtable[cc][i]);
  }
  j->pfx.resize((size_t)n);
  return JDS_OK;
}

static const char* const MCU_NOT_CODABLE =
    "not baseline-codable: a DC difference category above 11 or an AC category above 10";

// The Annex K table object on this thread's host side (and, with a context, on its device).
static int mcu_tables(jds_ctx* c, const char** host) {
  alignas(16) static thread_local char t[16384];
  static thread_local bool built = false;
  if (ent_tab_size() > sizeof t) return fail(JDS_EINVAL, "entropy tables exceed the staging buffer");
  if (!built) {
    ent_build_tables((EntTab*)t);
    built = true;
  }
  if (c && !c->ent_tab.p) {
    HIP_TRY(c->ent_tab.ensure(ent_tab_size()));
    HIP_TRY(hipMemcpy(c->ent_tab.p, t, ent_tab_size(), hipMemcpyHostToDevice));
  }
  *host = t;
  return JDS_OK;
}

static void mcu_std_tabs(McuStdTabs* t) {
  for (int i = 0; i < 4; ++i) t->n_vals[i] = ent_std_table(i, &t->bits[i], &t->vals[i]);
}

// The transformed files of a writer batch (DESIGN.md "Lossless transforms"):
// their records, tiles assigned, travel in the writer's upload and
// k_coef_xform runs in front of the writer's first kernel.
struct XfSet {
  std::vector<XfFile> files;
  int64_t tiles = 0;
  void add(XfFile f) {
    tiles += xf_set_tiles(&f, tiles);
    files.push_back(f);
  }
};

struct McuRun {
  McuDev d;
  int nf = 0, nseg = 0;
  std::vector<int64_t> len;  // per job: the file's bytes, 0: not baseline-codable
};

// The writer's launches up to the files' lengths, over the coefficients in
// c->ent_cf; the lengths and flags come back (the call's one read between the
// placement and the emit).
static int mcu_code(jds_ctx* c, std::vector<McuJob>& jobs, int optimize, McuRun* r, const XfSet* xf = nullptr) {
  hipStream_t s = c->stream;
  const int nf = (int)jobs.size();
  long long nseg = 0, raw_words = 0, pfx_bytes = 0;
  bool any_long = false;
  for (int k = 0; k < nf; ++k) {
    McuFile& f = jobs[(size_t)k].f;
    f.seg0 = (int32_t)nseg;
    f.frame = optimize ? k : 0;
    f.raw_w0 = raw_words;
    f.raw_words = mcu_raw_words(f.nblk);
    f.pfx_off = pfx_bytes;
    f.pfx_len = (int32_t)jobs[(size_t)k].pfx.size();
    if (f.gray) f.comp_id = mcu_gray_id(jobs[(size_t)k].pfx.data(), f.pfx_len);
    nseg += f.nseg;
    raw_words += f.raw_words;
    pfx_bytes += f.pfx_len;
    any_long = any_long || f.nseg > mcu_self_max();
    if (nseg > 0x1fffffffll || raw_words > 0x7fffffffll * 16)
      return fail(JDS_ENOTSUP, "batch of %d files: too many blocks for one set of writer launches", nf);
  }
  auto up = [](size_t v) { return (v + 255) & ~(size_t)255; };
  const size_t nxf = xf ? xf->files.size() : 0, nxt = xf ? (size_t)xf->tiles : 0;
  if (nxt > 0x7fffffffull) return fail(JDS_ENOTSUP, "batch of %d files: too many blocks for one transform launch", nf);
  const size_t o_seg = up(sizeof(McuFile) * (size_t)nf), o_pfx = up(o_seg + 4 * (size_t)nseg),
               o_xf = up(o_pfx + (size_t)pfx_bytes), o_xt = nxf ? up(o_xf + sizeof(XfFile) * nxf) : o_xf,
               total = nxf ? up(o_xt + 4 * nxt) : o_xf;
  std::vector<char> h(total, 0);
  for (size_t k = 0; k < nxf; ++k) {
    const XfFile& x = xf->files[k];
    memcpy(h.data() + o_xf + sizeof(XfFile) * k, &x, sizeof(XfFile));
    int32_t* tf = (int32_t*)(h.data() + o_xt) + x.tile0;
    const int64_t nt = (k + 1 < nxf ? (int64_t)xf->files[k + 1].tile0 : xf->tiles) - x.tile0;
    for (int64_t i = 0; i < nt; ++i) tf[i] = (int32_t)k;
  }
  for (int k = 0; k < nf; ++k) {
    const McuJob& j = jobs[(size_t)k];
    memcpy(h.data() + sizeof(McuFile) * (size_t)k, &j.f, sizeof(McuFile));
    int32_t* sf = (int32_t*)(h.data() + o_seg) + j.f.seg0;
    for (int i = 0; i < j.f.nseg; ++i) sf[i] = k;
    if (!j.pfx.empty()) memcpy(h.data() + o_pfx + j.f.pfx_off, j.pfx.data(), j.pfx.size());
  }
  const char* tab_host;
  int rc = mcu_tables(c, &tab_host);
  if (rc) return rc;
  HIP_TRY(c->mcu_up.ensure(total));
  HIP_TRY(c->mcu_scr.ensure(mcu_scratch_bytes(nf, nseg, raw_words)));
  McuDev& d = r->d;
  (void)mcu_carve(c->mcu_scr.p, nf, nseg, raw_words, &d);
  d.files = (const McuFile*)c->mcu_up.p;
  d.segfile = (const int32_t*)((const char*)c->mcu_up.p + o_seg);
  d.pfx = (const uint8_t*)c->mcu_up.p + o_pfx;
  // a header template: the DHT segments a table class falls back to (its other bytes are not used)
  uint8_t hdr[ENT_HDR];
  double ones[64];
  for (double& v : ones) v = 1.0;
  if (ent_header(ones, M444, 8, 8, hdr) != ENT_HDR) return fail(JDS_EINVAL, "header template");
  std::vector<char> frame(mcu_optframe_bytes());
  mcu_std_frame(ent_es_tab(tab_host), hdr, frame.data());
  HIP_TRY(hipMemcpyAsync(c->mcu_up.p, h.data(), total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(d.hdr_std, hdr, ENT_HDR, hipMemcpyHostToDevice, s));
  if (!optimize) HIP_TRY(hipMemcpyAsync(d.of, frame.data(), frame.size(), hipMemcpyHostToDevice, s));
  if (nxf)  // the transformed files' planes into the second coefficient region, where their McuFile points
    HIP_TRY(launch_coef_xform((const XfFile*)((const char*)c->mcu_up.p + o_xf),
                              (const int32_t*)((const char*)c->mcu_up.p + o_xt), (long long)nxt,
                              (const int16_t*)c->ent_cf.p, (int16_t*)c->ent_cf.p, s));
  HIP_TRY(launch_mcu_code(d, nf, (int)nseg, any_long, (const int16_t*)c->ent_cf.p, optimize != 0,
                          ent_es_tab(c->ent_tab.p), s));
  std::vector<unsigned long long> fl((size_t)nf);
  std::vector<uint32_t> fb((size_t)nf);
  HIP_TRY(hipMemcpyAsync(fl.data(), d.flen, 8 * (size_t)nf, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(fb.data(), d.fbad, 4 * (size_t)nf, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));  // (h, hdr and frame are this call's objects)
  r->nf = nf;
  r->nseg = (int)nseg;
  r->len.assign((size_t)nf, 0);
  for (int k = 0; k < nf; ++k) {
    if ((long long)fl[(size_t)k] > mcu_capacity(jobs[(size_t)k].f) || fl[(size_t)k] < 4)
      return fail(JDS_EHIP, "writer: file %d reports %llu bytes, outside its bound", k, fl[(size_t)k]);
    r->len[(size_t)k] = fb[(size_t)k] ? 0 : (int64_t)fl[(size_t)k];
  }
  return JDS_OK;
}

// The files at fout (per job; < 0: not written) into out_dev; asynchronous on the context's stream.
static int mcu_emit(jds_ctx* c, const McuRun& r, const std::vector<long long>& fout, uint8_t* out_dev) {
  HIP_TRY(hipMemcpyAsync(r.d.fout, fout.data(), 8 * (size_t)r.nf, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(launch_mcu_emit(r.d, r.nf, r.nseg, out_dev, c->stream));
  return JDS_OK;
}

// One job whose coefficients are in c->ent_cf, to host memory.
static int mcu_single(jds_ctx* c, McuJob& job, int32_t optimize, uint8_t* out, int64_t out_cap, int64_t* out_len,
                      const XfSet* xf = nullptr) {
  std::vector<McuJob> jobs(1);
  jobs[0] = std::move(job);
  McuRun r;
  const CtxMarkScope marks_(c, c->stream);
  int rc = mcu_code(c, jobs, optimize, &r, xf);
  if (rc) return rc;
  if (r.len[0] == 0) return fail(JDS_EINVAL, "%s", MCU_NOT_CODABLE);
  *out_len = r.len[0];
  if (r.len[0] > out_cap || !out)
    return fail(JDS_EINVAL, "output buffer too small: %lld bytes needed", (long long)r.len[0]);
  HIP_TRY(c->ent_out.ensure((size_t)r.len[0]));
  const std::vector<long long> fout(1, 0ll);
  if ((rc = mcu_emit(c, r, fout, (uint8_t*)c->ent_out.p))) return rc;
  HIP_TRY(hipMemcpyAsync(out, c->ent_out.p, (size_t)r.len[0], hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(hipStreamSynchronize(c->stream));
  return JDS_OK;
}

int jds_encode_jpeg(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, int32_t optimize,
                    const uint8_t* prefix, int64_t prefix_len, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  if (!c || !info || !coeffs || !out_len) return fail(JDS_EINVAL, "null argument");
  McuJob job;
  int rc;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  if ((rc = mcu_job_prefix(info, prefix, prefix_len, &job))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nbytes = (size_t)mcu_coeffs(job.f) * sizeof(int16_t);
  HIP_TRY(c->ent_cf.ensure(nbytes));
  HIP_TRY(hipMemcpyAsync(c->ent_cf.p, coeffs, nbytes, hipMemcpyHostToDevice, c->stream));
  return mcu_single(c, job, optimize, out, out_cap, out_len);
}

int jds_jpeg_transcode(jds_ctx* c, const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out, int64_t out_cap,
                       int64_t* out_len, jds_jpeg_info* info) {
  if (!c || !data || !info || !out_len) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  McuJob job;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  if ((rc = mcu_job_splice(data, len, &job))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_jpeg_dev(c, data, len, info))) return rc;  // (a defective scan: nothing is written)
  return mcu_single(c, job, optimize, out, out_cap, out_len);
}

// One file's transform, settled on the host before anything runs: the
// operation (JDS_XF_AUTO resolved from the spliced prefix), its geometry and
// the prefix, edited unless the operation is none.
struct XfJob {
  int op = JDS_XF_NONE;
  XfPlan plan;
  std::vector<uint8_t> pfx;
};

static inline int64_t xf_align(int64_t entries) { return (entries + 127) & ~(int64_t)127; }

static int xf_prepare(const uint8_t* data, int64_t len, const jds_jpeg_info* info, int32_t op_in, XfJob* x) {
  const int base = op_in & 0xFF;
  if (op_in < 0 || (op_in & ~(0xFF | JDS_XF_TRIM)) || base > JDS_XF_AUTO)
    return fail(JDS_EINVAL, "unknown transform operation 0x%x", (unsigned)op_in);
  McuJob sp;
  int rc = mcu_job_splice(data, len, &sp);
  if (rc) return rc;
  x->pfx = std::move(sp.pfx);
  int64_t pos = -1;
  int big = 0, op = base;
  if (base == JDS_XF_AUTO)
    op = xf_op_of_orientation(xf_exif_orientation(x->pfx.data(), (int64_t)x->pfx.size(), &pos, &big));
  char msg[320];
  if ((rc = xf_plan(info, op, (op_in & JDS_XF_TRIM) != 0, &x->plan, msg, sizeof msg))) return fail(rc, "%s", msg);
  x->op = op;
  if (op == JDS_XF_NONE) return JDS_OK;
  const int e = xf_edit_prefix(x->pfx.data(), (int64_t)x->pfx.size(), x->plan.flags, x->plan.dst.H, x->plan.dst.W);
  if (e == -2) return fail(JDS_ENOTSUP, "DQT: a 16-bit or incomplete table cannot be transposed");
  if (e) return fail(JDS_EINVAL, "header prefix: %s", e == -3 ? "no SOF0 segment" : "not a sequence of marker segments");
  if (pos >= 0) xf_exif_reset(x->pfx.data(), pos, big);
  return JDS_OK;
}

// jds_jpeg_batch_transcode, and with `xform` jds_jpeg_batch_transform: the same
// launches with per-file transformed records handed to the writer's driver.
static int batch_transcode(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n, bool xform,
                           const int32_t* ops, int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                           jds_jpeg_transcode_item* items, int64_t* out_bytes) {
  if (!c || !out_bytes || (n > 0 && !items)) return fail(JDS_EINVAL, "null argument");
  *out_bytes = 0;
  std::vector<jds_jpeg_batch_item> bi((size_t)(n > 0 ? n : 0));
  BatchPlan bp;
  int rc = batch_layout(data, lens, n, bi.data(), bp);
  if (rc) return rc;
  // the transformed planes follow the decoder's in c->ent_cf: sized before the decode fills it
  std::vector<XfJob> xj((size_t)(xform && n > 0 ? n : 0));
  const int64_t xbase = xf_align(bp.coef_entries);
  int64_t xtotal = 0;
  for (int i = 0; xform && i < n; ++i) {
    if (bp.rec_of[(size_t)i] < 0) continue;
    XfJob& x = xj[(size_t)i];
    const int rc1 = xf_prepare(data[i], lens[i], &bp.info[(size_t)i], ops ? ops[i] : JDS_XF_AUTO, &x);
    if (rc1) {  // refused: an item error with the code the file would get alone
      bi[(size_t)i].rc = rc1;
      if (bp.first_bad < 0 || i < bp.first_bad) {
        bp.first_bad = i;
        snprintf(bp.first_msg, sizeof bp.first_msg, "%s", g_err);
      }
      continue;
    }
    bi[(size_t)i].H = x.plan.dst.H;
    bi[(size_t)i].W = x.plan.dst.W;
    if (x.op != JDS_XF_NONE) xtotal += xf_align(x.plan.dst.coeffs_needed);
  }
  if (xtotal) {
    HIP_TRY(hipSetDevice(c->device));
    HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)(xbase + xtotal)));
  }
  if (!bp.recs.empty() && (rc = batch_run(c, bp, data, lens, nullptr, 0, nullptr, bi.data(), nullptr, false)))
    return rc;
  for (int i = 0; i < n; ++i) {
    jds_jpeg_transcode_item& it = items[i];
    memset(&it, 0, sizeof it);
    it.rc = bi[(size_t)i].rc;
    it.status = bi[(size_t)i].status;
    it.H = bi[(size_t)i].H;
    it.W = bi[(size_t)i].W;
    it.subsampling = bi[(size_t)i].subsampling;
    it.interleaved = bi[(size_t)i].interleaved;
    it.out_off = -1;
  }
  // the files that decoded take part in the writer's launches
  std::vector<McuJob> jobs;
  std::vector<int> job_file;
  XfSet xs;
  int64_t xcur = xbase;
  for (size_t k = 0; k < bp.recs.size(); ++k) {
    const int i = bp.file_of[k];
    if (items[i].status || items[i].rc) continue;
    McuJob j;
    if (xform && xj[(size_t)i].op != JDS_XF_NONE) {  // the writer sees the destination planes
      XfJob& x = xj[(size_t)i];
      if ((rc = mcu_job_geo(&x.plan.dst, xcur, &j))) return rc;
      XfFile rec = x.plan.rec;
      for (int cc = 0; cc < 3; ++cc) {
        rec.soff[cc] += bp.recs[k].coef_off;
        rec.doff[cc] += xcur;
      }
      xs.add(rec);
      xcur += xf_align(x.plan.dst.coeffs_needed);
      j.pfx = std::move(x.pfx);
    } else {
      if ((rc = mcu_job_geo(&bp.info[(size_t)i], bp.recs[k].coef_off, &j))) return rc;
      if ((rc = mcu_job_splice(data[i], lens[i], &j))) return rc;
    }
    jobs.push_back(std::move(j));
    job_file.push_back(i);
  }
  if (jobs.empty()) {
    batch_note(bp);
    return JDS_OK;
  }
  hipStream_t s = c->stream;
  const CtxMarkScope marks_(c, s);
  McuRun r;
  if ((rc = mcu_code(c, jobs, optimize, &r, xs.files.empty() ? nullptr : &xs))) return rc;
  std::vector<long long> fout(jobs.size(), -1ll);
  int64_t cur = 0;
  for (size_t k = 0; k < jobs.size(); ++k) {
    const int i = job_file[k];
    if (r.len[k] == 0) {
      items[i].rc = fail(JDS_EINVAL, "%s", MCU_NOT_CODABLE);
      if (bp.first_bad < 0 || i < bp.first_bad) {
        bp.first_bad = i;
        snprintf(bp.first_msg, sizeof bp.first_msg, "%s", MCU_NOT_CODABLE);
      }
      continue;
    }
    fout[k] = cur;
    items[i].out_off = cur;
    items[i].out_len = r.len[k];
    cur = (cur + r.len[k] + 255) & ~(int64_t)255;
  }
  *out_bytes = cur;
  if (cur > 0 && (!out || out_cap < cur))
    return fail(JDS_EINVAL, "output buffer too small: %lld bytes needed", (long long)cur);
  if (cur > 0) {
    uint8_t* dst = out;
    if (!out_on_device) {
      HIP_TRY(c->ent_out.ensure((size_t)cur));
      dst = (uint8_t*)c->ent_out.p;
    }
    if ((rc = mcu_emit(c, r, fout, dst))) return rc;
    if (!out_on_device)  // file by file: the gaps of the caller's buffer stay as they are
      for (size_t k = 0; k < jobs.size(); ++k)
        if (fout[k] >= 0)
          HIP_TRY(hipMemcpyAsync(out + fout[k], dst + fout[k], (size_t)r.len[k], hipMemcpyDeviceToHost, s));
    kmark(s, "(transcode download)");
    HIP_TRY(hipStreamSynchronize(s));
  }
  batch_note(bp);
  return JDS_OK;
}

int jds_jpeg_batch_transcode(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n,
                             int32_t optimize, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                             jds_jpeg_transcode_item* items, int64_t* out_bytes) {
  return batch_transcode(c, data, lens, n, false, nullptr, optimize, out, out_cap, out_on_device, items, out_bytes);
}

// ------------------------------------------------ lossless transforms --
// (DESIGN.md "Lossless transforms"; kernel: jds_xform.hip; host side: jds_xform.hpp)

int jds_jpeg_batch_transform(jds_ctx* c, const uint8_t* const* data, const int64_t* lens, int32_t n,
                             const int32_t* ops, int32_t optimize, uint8_t* out, int64_t out_cap,
                             int32_t out_on_device, jds_jpeg_transcode_item* items, int64_t* out_bytes) {
  return batch_transcode(c, data, lens, n, true, ops, optimize, out, out_cap, out_on_device, items, out_bytes);
}

int jds_jpeg_transform_info(const uint8_t* data, int64_t len, int32_t op, int32_t* op_out, int64_t* H_out,
                            int64_t* W_out) {
  if (!data || !op_out || !H_out || !W_out) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info info;
  int rc = jds_jpeg_parse(data, len, &info);
  if (rc) return rc;
  XfJob x;
  if ((rc = xf_prepare(data, len, &info, op, &x))) return rc;
  *op_out = x.op;
  *H_out = x.plan.dst.H;
  *W_out = x.plan.dst.W;
  return JDS_OK;
}

int jds_jpeg_transform(jds_ctx* c, const uint8_t* data, int64_t len, int32_t op, int32_t optimize, uint8_t* out,
                       int64_t out_cap, int64_t* out_len, jds_jpeg_info* info) {
  if (!c || !data || !info || !out_len) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jpeg_parse(data, len, info);
  if (rc) return rc;
  XfJob x;
  if ((rc = xf_prepare(data, len, info, op, &x))) return rc;
  McuJob job;
  if (x.op == JDS_XF_NONE) {  // jds_jpeg_transcode
    if ((rc = mcu_job_geo(info, 0, &job))) return rc;
    job.pfx = std::move(x.pfx);
    HIP_TRY(hipSetDevice(c->device));
    if ((rc = decode_jpeg_dev(c, data, len, info))) return rc;
    return mcu_single(c, job, optimize, out, out_cap, out_len);
  }
  const int64_t base = xf_align(info->coeffs_needed);
  if ((rc = mcu_job_geo(&x.plan.dst, base, &job))) return rc;
  job.pfx = std::move(x.pfx);
  XfFile rec = x.plan.rec;
  for (int cc = 0; cc < 3; ++cc) rec.doff[cc] += base;
  XfSet xs;
  xs.add(rec);
  HIP_TRY(hipSetDevice(c->device));
  // the transformed planes follow the decoder's: sized before the decode fills the buffer
  HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)(base + x.plan.dst.coeffs_needed)));
  if ((rc = decode_jpeg_dev(c, data, len, info))) return rc;  // (a defective scan: nothing is written)
  return mcu_single(c, job, optimize, out, out_cap, out_len, &xs);
}

int jds_selftest_coef_transform_dev(jds_ctx* c, const jds_jpeg_info* info, int32_t op, const int16_t* coeffs,
                                    int16_t* coeffs_out) {
  if (!c || !info || !coeffs || !coeffs_out) return fail(JDS_EINVAL, "null argument");
  const int base_op = op & 0xFF;
  if (op < 0 || (op & ~(0xFF | JDS_XF_TRIM)) || base_op >= JDS_XF_AUTO)
    return fail(JDS_EINVAL, "unknown transform operation 0x%x (an explicit operation is needed)", (unsigned)op);
  XfPlan p;
  char msg[320];
  int rc = xf_plan(info, base_op, (op & JDS_XF_TRIM) != 0, &p, msg, sizeof msg);
  if (rc) return fail(rc, "%s", msg);
  McuFile sf;
  (void)mcu_file_of(info, &sf);  // (xf_plan has checked it)
  const int64_t nsrc = mcu_coeffs(sf), base = xf_align(nsrc), ndst = p.dst.coeffs_needed;
  XfFile rec = p.rec;
  for (int cc = 0; cc < 3; ++cc) rec.doff[cc] += base;
  const size_t o_t = (sizeof(XfFile) + 255) & ~(size_t)255, total = o_t + 4 * (size_t)p.tiles;
  std::vector<char> h(total, 0);  // (the tile table: every tile is record 0's)
  memcpy(h.data(), &rec, sizeof rec);
  hipStream_t s = c->stream;
  HIP_TRY(hipSetDevice(c->device));
  HIP_TRY(c->mcu_up.ensure(total));
  HIP_TRY(c->ent_cf.ensure(sizeof(int16_t) * (size_t)(base + ndst)));
  int16_t* cf = (int16_t*)c->ent_cf.p;
  HIP_TRY(hipMemcpyAsync(c->mcu_up.p, h.data(), total, hipMemcpyHostToDevice, s));
  HIP_TRY(hipMemcpyAsync(cf, coeffs, sizeof(int16_t) * (size_t)nsrc, hipMemcpyHostToDevice, s));
  HIP_TRY(launch_coef_xform((const XfFile*)c->mcu_up.p, (const int32_t*)((const char*)c->mcu_up.p + o_t),
                            (long long)p.tiles, cf, cf, s));
  HIP_TRY(hipMemcpyAsync(coeffs_out, cf + base, sizeof(int16_t) * (size_t)ndst, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  return JDS_OK;
}

// the host model's result into the caller's buffer
static int mcu_host_result(int wrc, const std::vector<uint8_t>& file, uint8_t* out, int64_t out_cap,
                           int64_t* out_len) {
  if (wrc) return fail(JDS_EINVAL, "%s", MCU_NOT_CODABLE);
  *out_len = (int64_t)file.size();
  if (!out || out_cap < (int64_t)file.size())
    return fail(JDS_EINVAL, "output buffer too small: %lld bytes needed", (long long)file.size());
  memcpy(out, file.data(), file.size());
  return JDS_OK;
}

int jds_selftest_jpeg_transcode(const uint8_t* data, int64_t len, int32_t optimize, uint8_t* out, int64_t out_cap,
                                int64_t* out_len) {
  if (!data || !out_len) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info info;
  int rc = jds_jpeg_parse(data, len, &info);
  if (rc) return rc;
  McuJob job;
  if ((rc = mcu_job_geo(&info, 0, &job))) return rc;
  if ((rc = mcu_job_splice(data, len, &job))) return rc;
  int lane_max, sb, spg;
  rst_constants(&lane_max);
  dec_constants(&sb, &spg);
  std::vector<int16_t> cf((size_t)info.coeffs_needed);
  int32_t rounds[3];
  const uint32_t st = hd_jpeg_host_decode(data, &info, sb, lane_max, cf.data(), rounds);
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  McuStdTabs std_tabs;
  mcu_std_tabs(&std_tabs);
  std::vector<uint8_t> file;
  const int wrc = mcu_host_write(job.f, cf.data(), optimize, job.pfx.data(), (int64_t)job.pfx.size(), std_tabs, &file);
  return mcu_host_result(wrc, file, out, out_cap, out_len);
}

int jds_selftest_jpeg_transform(const uint8_t* data, int64_t len, int32_t op, int32_t optimize, uint8_t* out,
                                int64_t out_cap, int64_t* out_len) {
  if (!data || !out_len) return fail(JDS_EINVAL, "null argument");
  jds_jpeg_info info;
  int rc = jds_jpeg_parse(data, len, &info);
  if (rc) return rc;
  XfJob x;
  if ((rc = xf_prepare(data, len, &info, op, &x))) return rc;
  McuJob job;
  if ((rc = mcu_job_geo(x.op == JDS_XF_NONE ? &info : &x.plan.dst, 0, &job))) return rc;
  int lane_max, sb, spg;
  rst_constants(&lane_max);
  dec_constants(&sb, &spg);
  std::vector<int16_t> cf((size_t)info.coeffs_needed);
  int32_t rounds[3];
  const uint32_t st = hd_jpeg_host_decode(data, &info, sb, lane_max, cf.data(), rounds);
  if (st) return fail(JDS_EINVAL, "defective scan data: %s (status 0x%x)", hd_status_text(st), st);
  if (x.op != JDS_XF_NONE) {
    std::vector<int16_t> dst((size_t)x.plan.dst.coeffs_needed);
    xf_host(x.plan.rec, cf.data(), dst.data());
    cf.swap(dst);
  }
  McuStdTabs std_tabs;
  mcu_std_tabs(&std_tabs);
  std::vector<uint8_t> file;
  const int wrc = mcu_host_write(job.f, cf.data(), optimize, x.pfx.data(), (int64_t)x.pfx.size(), std_tabs, &file);
  return mcu_host_result(wrc, file, out, out_cap, out_len);
}

int jds_selftest_jpeg_encode(const jds_jpeg_info* info, const int16_t* coeffs, int32_t optimize, const uint8_t* prefix,
                             int64_t prefix_len, uint8_t* out, int64_t out_cap, int64_t* out_len) {
  if (!info || !coeffs || !out_len) return fail(JDS_EINVAL, "null argument");
  McuJob job;
  int rc;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  if ((rc = mcu_job_prefix(info, prefix, prefix_len, &job))) return rc;
  McuStdTabs std_tabs;
  mcu_std_tabs(&std_tabs);
  std::vector<uint8_t> file;
  const int wrc = mcu_host_write(job.f, coeffs, optimize, job.pfx.data(), (int64_t)job.pfx.size(), std_tabs, &file);
  return mcu_host_result(wrc, file, out, out_cap, out_len);
}

int jds_selftest_jpeg_hist_dev(jds_ctx* c, const jds_jpeg_info* info, const int16_t* coeffs, uint32_t* counts) {
  if (!c || !info || !coeffs || !counts) return fail(JDS_EINVAL, "null argument");
  McuJob job;
  int rc;
  if ((rc = mcu_job_geo(info, 0, &job))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  const size_t nbytes = (size_t)mcu_coeffs(job.f) * sizeof(int16_t);
  HIP_TRY(c->ent_cf.ensure(nbytes));
  HIP_TRY(hipMemcpyAsync(c->ent_cf.p, coeffs, nbytes, hipMemcpyHostToDevice, c->stream));
  std::vector<McuJob> jobs(1);
  jobs[0] = std::move(job);
  McuRun r;
  if ((rc = mcu_code(c, jobs, 1, &r))) return rc;
  // (the counters open the file's frame)
  HIP_TRY(hipMemcpy(counts, r.d.of, sizeof(uint32_t) * 2 * OPT_BINS, hipMemcpyDeviceToHost));
  return JDS_OK;
}

int jds_decompress_jfif(jds_ctx* c, const uint8_t* data, int64_t len, uint8_t* rgb_out, int64_t rgb_cap,
                        int16_t* coeffs, jds_jfif_info* info) {
  if (!c || !data || !info || !rgb_out) return fail(JDS_EINVAL, "null argument");
  int rc = jds_jfif_parse(data, len, info);
  if (rc) return rc;
  const size_t nimg = (size_t)info->H * (size_t)info->W * 3;
  if (rgb_cap < (int64_t)nimg) return fail(JDS_EINVAL, "image buffer too small: %zu bytes needed", nimg);
  jds_params prm;
  memset(&prm, 0, sizeof prm);
  prm.block_size = 8;
  prm.quality = 0;
  prm.subsampling = info->subsampling;
  memcpy(prm.qtable, info->qtable, sizeof prm.qtable);
  if ((rc = check_tables(&prm))) return rc;
  HIP_TRY(hipSetDevice(c->device));
  if ((rc = decode_file_dev(c, data, len, info))) return rc;
  return inverse_of_decoded(c, &prm, info->H, info->W, info->coeffs_needed, rgb_out, coeffs);
}

// c->ent_cf (a decoded frame) -> rgb_out by the plan's default inverse route for
// this geometry and table, on zeroed statistics; coeffs: NULL or n_coeffs entries.
static int inverse_of_decoded(jds_ctx* c, const jds_params* prm, int64_t H, int64_t W, int64_t n_coeffs,
                              uint8_t* rgb_out, int16_t* coeffs) {
  const size_t nimg = (size_t)H * (size_t)W * 3;
  int rc;
  jds_plan* plan = nullptr;
  if ((rc = jds_plan_create(c, prm, 1, H, W, &plan))) return rc;
  hipError_t e;
  if ((e = c->rgb.ensure(nimg)) != hipSuccess || (e = c->out.ensure(nimg)) != hipSuccess ||
      (e = c->stats.ensure(sizeof(jds_frame_stats))) != hipSuccess ||
      (e = hipMemsetAsync(c->stats.p, 0, sizeof(jds_frame_stats), c->stream)) != hipSuccess) {
    jds_plan_destroy(plan);
    return fail(e == hipErrorOutOfMemory ? JDS_ENOMEM : JDS_EHIP, "decompress: %s", hipGetErrorString(e));
  }
  rc = jds_plan_run(plan, (const uint8_t*)c->rgb.p, (uint8_t*)c->out.p, (int16_t*)c->ent_cf.p,
                    (jds_frame_stats*)c->stats.p, JDS_RUN_INV, c->stream);
  if (rc == JDS_OK) {
    e = hipMemcpyAsync(rgb_out, c->out.p, nimg, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess && coeffs)
      e = hipMemcpyAsync(coeffs, c->ent_cf.p, (size_t)n_coeffs * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) rc = fail(JDS_EHIP, "decompress: %s", hipGetErrorString(e));
  }
  jds_plan_destroy(plan);  // (waits for the context's stream)
  return rc;
}

int jds_plan_entropy_decode(jds_plan* p, const uint8_t* files, int64_t stride, const uint64_t* lengths,
                            int16_t* coeffs, uint32_t* status, void* stream) {
  if (!p || !files || !lengths || !coeffs || !status) return fail(JDS_EINVAL, "null argument");
  if (stride < 1) return fail(JDS_EINVAL, "stride %lld", (long long)stride);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t s = (hipStream_t)stream;
  if (!p->ent_hdr.p) {
    int rc = ent_prepare(p->g, p->mode, p->n, p->qt, p->ent, p->ent_hdr, p->ent_tab, s);
    if (rc) return rc;
  }
  const MarkScope marks_(p, s);
  size_t sz[8];
  ent_sizes(p->g, p->n, sz);
  const int hl = (int)(sz[6] / (size_t)p->n);
  if (!p->dec_tab.p) {
    // the decode tables come from the DHT segments of the plan's own header
    std::vector<uint8_t> h((size_t)hl);
    jds_jfif_info hi;
    if (ent_header(p->qt, p->mode, p->g.H, p->g.W, h.data()) != hl ||
        hd_parse(h.data(), hl, &hi, true, g_err, sizeof g_err) != JDS_OK)
      return fail(JDS_EINVAL, "entropy decode: the plan's header template does not parse");
    HuffDecTab tabs[4];
    for (int i = 0; i < 4; ++i)
      if (!hi.huff[i].defined || hd_build(hi.huff[i].bits, hi.huff[i].vals, &tabs[i]) < 0)
        return fail(JDS_EINVAL, "entropy decode: the plan's header template lacks a Huffman table");
    HIP_TRY(p->dec_tab.ensure(sizeof tabs));
    HIP_TRY(hipMemcpy(p->dec_tab.p, tabs, sizeof tabs, hipMemcpyHostToDevice));
  }
  const int n = p->n;
  if (n > 65535) return fail(JDS_ENOTSUP, "entropy decode: at most 65535 frames per call");
  HIP_TRY(p->dec_info.ensure(dec_hdr_bytes(n)));
  HIP_TRY(launch_dec_hdr(files, stride, (const unsigned long long*)lengths, (const uint8_t*)p->ent_hdr.p, hl, n,
                         p->dec_info.p, status, s));
  std::vector<long long> si(6 * (size_t)n);
  std::vector<uint32_t> st((size_t)n);
  HIP_TRY(hipMemcpyAsync(si.data(), p->dec_info.p, sizeof(long long) * si.size(), hipMemcpyDeviceToHost, s));
  HIP_TRY(hipMemcpyAsync(st.data(), status, 4 * (size_t)n, hipMemcpyDeviceToHost, s));
  HIP_TRY(hipStreamSynchronize(s));
  const long long nyb = (long long)p->g.nby * p->g.nbx, ncb = (long long)p->g.ncy * p->g.ncx;
  std::vector<DecScan> sc(3 * (size_t)n);
  for (int f = 0; f < n; ++f)
    for (int k = 0; k < 3; ++k) {
      DecScan& d = sc[3 * (size_t)f + k];
      d = DecScan{};
      d.frame = f;
      d.dc_tab = k ? 1 : 0;
      d.ac_tab = k ? 3 : 2;
      d.coef_off = (long long)f * p->g.cpf + (k == 0 ? 0 : (k == 1 ? p->g.off_cb : p->g.off_cr));
      if (st[f]) continue;  // skipped frame: no workgroups
      d.data_off = (long long)f * stride + si[6 * (size_t)f + 2 * k];
      d.nbytes = si[6 * (size_t)f + 2 * k + 1];
      d.nblocks = (int)(k ? ncb : nyb);
    }
  int max_ngrp = 0;
  const long long ng = dec_layout(sc.data(), 3 * n, &max_ngrp);
  if (ng < 0) return fail(JDS_ENOTSUP, "batch too long for one decode");
  HIP_TRY(p->dec_scr.ensure(dec_scratch_bytes(ng, 3 * n)));
  int too_many = 0;
  p->dec_rounds = 0;
  HIP_TRY(dec_run(files, sc.data(), 3 * n, ng, max_ngrp, (const HuffDecTab*)p->dec_tab.p, p->dec_scr.p, coeffs,
                  (long long)n * p->g.cpf, status, s, &p->dec_rounds, &too_many, nullptr, nullptr));
  if (too_many) return fail(JDS_EHIP, "entropy decode: propagation did not settle within %d rounds", max_ngrp);
  return JDS_OK;
}

int jds_plan_entropy_decode_rst(jds_plan* p, int32_t interval, const uint8_t* files, int64_t stride,
                                const uint64_t* lengths, int16_t* coeffs, uint32_t* status, void* stream) {
  if (!p || !files || !lengths || !coeffs || !status) return fail(JDS_EINVAL, "null argument");
  if (stride < 1) return fail(JDS_EINVAL, "stride %lld", (long long)stride);
  int lane_max;
  rst_constants(&lane_max);
  if (interval == 0)
    return fail(JDS_EINVAL, "restart interval 0: jds_plan_entropy_decode reads files without restart markers");
  if (interval < 0 || interval > lane_max)
    return fail(JDS_ENOTSUP, "restart interval %d: the batch decode takes 1 .. %d", interval, lane_max);
  HIP_TRY(hipSetDevice(p->ctx->device));
  hipStream_t s = (hipStream_t)stream;
  // everything below that waits happens once per plan (and interval); a repeated call only enqueues
  if (!p->ent_hdr.p) {
    int rc = ent_prepare(p->g, p->mode, p->n, p->qt, p->ent, p->ent_hdr, p->ent_tab, s);
    if (rc) return rc;
  }
  const int n = p->n;
  size_t sz[8];
  ent_sizes(p->g, n, sz);
  const int hl0 = (int)(sz[6] / (size_t)n), hl = hl0 + 6;
  if (!p->dec_tab.p) {
    std::vector<uint8_t> h((size_t)hl0);
    jds_jfif_info hi;
    if (ent_header(p->qt, p->mode, p->g.H, p->g.W, h.data()) != hl0 ||
        hd_parse(h.data(), hl0, &hi, true, g_err, sizeof g_err) != JDS_OK)
      return fail(JDS_EINVAL, "entropy decode: the plan's header template does not parse");
    HuffDecTab tabs[4];
    for (int i = 0; i < 4; ++i)
      if (!hi.huff[i].defined || hd_build(hi.huff[i].bits, hi.huff[i].vals, &tabs[i]) < 0)
        return fail(JDS_EINVAL, "entropy decode: the plan's header template lacks a Huffman table");
    HIP_TRY(p->dec_tab.ensure(sizeof tabs));
    HIP_TRY(hipMemcpy(p->dec_tab.p, tabs, sizeof tabs, hipMemcpyHostToDevice));
  }
  if (p->rst_hdr_interval != interval) {
    std::vector<uint8_t> h((size_t)hl * (size_t)n);
    for (int i = 0; i < n; ++i)
      if (ent_header_rst(p->qt + 64 * i, p->mode, p->g.H, p->g.W, interval, h.data() + (size_t)hl * i) != hl)
        return fail(JDS_EINVAL, "frame %d: baseline JPEG needs integer quantisation steps in [1, 255]", i);
    HIP_TRY(p->rst_hdr.ensure(h.size()));
    HIP_TRY(hipMemcpy(p->rst_hdr.p, h.data(), h.size(), hipMemcpyHostToDevice));
    p->rst_hdr_interval = interval;
  }
  RstGeo rg{};
  rg.ri = interval;
  rg.nblk[0] = p->g.nby * p->g.nbx;
  rg.nblk[1] = rg.nblk[2] = p->g.ncy * p->g.ncx;
  rg.first[0] = 0;
  for (int k = 0; k < 3; ++k) rg.first[k + 1] = rg.first[k] + (rg.nblk[k] + interval - 1) / interval;
  rg.off[0] = 0;
  rg.off[1] = p->g.off_cb;
  rg.off[2] = p->g.off_cr;
  rg.cpf = p->g.cpf;
  if ((long long)rg.first[3] * n > 0x7fffffffll) return fail(JDS_ENOTSUP, "batch too long for one decode");
  HIP_TRY(p->rst_work.ensure(rst_work_bytes(n, rg)));
  const MarkScope marks_(p, s);
  p->dec_rounds = 0;
  HIP_TRY(launch_dec_rst_plan(files, stride, (const unsigned long long*)lengths, (const uint8_t*)p->rst_hdr.p, hl, n, rg,
                              p->rst_work.p, (const HuffDecTab*)p->dec_tab.p, coeffs, status, s));
  return JDS_OK;
}

int jds_plan_entropy_decode_rounds(const jds_plan* p, uint32_t* rounds) {
  if (!p || !rounds) return fail(JDS_EINVAL, "null argument");
  *rounds = p->dec_rounds;
  return JDS_OK;
}

int jds_selftest_dct8x8(const double* in, double* out, int64_t n, int32_t inverse) {
  if (!in || !out || n < 0) return fail(JDS_EINVAL, "bad argument");
  for (int64_t b = 0; b < n; ++b) {
    double t[64];
    memcpy(t, in + 64 * b, sizeof t);
    for (int col = 0; col < 8; ++col) {  // axis 0 first
      double* c = t + col;
      if (inverse)
        dct3_line(c[0], c[8], c[16], c[24], c[32], c[40], c[48], c[56]);
      else
        dct2_line(c[0], c[8], c[16], c[24], c[32], c[40], c[48], c[56]);
    }
    for (int r = 0; r < 8; ++r) {
      double* c = t + 8 * r;
      if (inverse)
        dct3_line(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
      else
        dct2_line(c[0], c[1], c[2], c[3], c[4], c[5], c[6], c[7]);
    }
    for (int i = 0; i < 64; ++i) out[64 * b + i] = t[i] * 0.0625;  // pocketfft fct = 1/16
  }
  return JDS_OK;
}

int jds_selftest_fwd32(int32_t subsampling, int32_t prefilter, const double* gauss, const uint8_t* rgb, int64_t H,
                       int64_t W, int32_t plane, int32_t rows_first, float* coeffs, double* bound) {
  if (!gauss || !rgb || !coeffs || !bound || H < 1 || W < 1 || H > 4096 || W > 4096 || plane < 0 || plane > 2 ||
      subsampling < JDS_SS_444 || subsampling > JDS_SS_420)
    return fail(JDS_EINVAL, "bad argument");
  const bool pf = prefilter != 0 && subsampling != JDS_SS_444;
  double E[128];
  fast_fwd_bounds(subsampling, pf, gauss, E);
  memcpy(bound, E + (plane ? 64 : 0), 64 * sizeof(double));
  if (fwd32_host_plane(subsampling, pf, gauss, rgb, (int)H, (int)W, plane, rows_first, coeffs))
    return fail(JDS_EINVAL, "plane size must be a multiple of 8");
  return JDS_OK;
}

int jds_selftest_fwd16(int32_t subsampling, int32_t prefilter, const double* gauss, const uint8_t* rgb, int64_t H,
                       int64_t W, int32_t plane, int32_t rows_first, float* coeffs, double* bound) {
  if (!gauss || !rgb || !coeffs || !bound || H < 1 || W < 1 || H > 4096 || W > 4096 || plane < 0 || plane > 2 ||
      subsampling < JDS_SS_444 || subsampling > JDS_SS_420)
    return fail(JDS_EINVAL, "bad argument");
  const bool pf = prefilter != 0 && subsampling != JDS_SS_444;
  double E[512];
  fast_fwd16_bounds(subsampling, pf, gauss, E);
  memcpy(bound, E + (plane ? 256 : 0), 256 * sizeof(double));
  if (fwd16_host_plane(subsampling, pf, gauss, rgb, (int)H, (int)W, plane, rows_first, coeffs))
    return fail(JDS_EINVAL, "plane size must be a multiple of 16");
  return JDS_OK;
}

int jds_selftest_inv_fast(int32_t subsampling, const int16_t* coeffs, const double* qtable, int64_t H, int64_t W,
                          int32_t fuse, double* values, uint8_t* bytes) {
  if (!coeffs || !qtable || !values || !bytes || H < 1 || W < 1 || H > 4096 || W > 4096 ||
      subsampling < JDS_SS_444 || subsampling > JDS_SS_420)
    return fail(JDS_EINVAL, "bad argument");
  if (inv_fast_host(subsampling, coeffs, qtable, (int)H, (int)W, fuse, 8, values, bytes))
    return fail(JDS_EINVAL, "odd chroma geometry: the certified inverse runs even sizes only");
  return JDS_OK;
}

int jds_selftest_inv_fast16(int32_t subsampling, const int16_t* coeffs, const double* qtable, int64_t H, int64_t W,
                            int32_t fuse, double* values, uint8_t* bytes) {
  if (!coeffs || !qtable || !values || !bytes || H < 1 || W < 1 || H > 4096 || W > 4096 ||
      subsampling < JDS_SS_444 || subsampling > JDS_SS_420)
    return fail(JDS_EINVAL, "bad argument");
  if (inv_fast_host(subsampling, coeffs, qtable, (int)H, (int)W, fuse, 16, values, bytes))
    return fail(JDS_EINVAL, "odd chroma geometry: the certified inverse runs even sizes only");
  return JDS_OK;
}

int jds_selftest_area_tab(int32_t src, int32_t dst, int32_t* n, int32_t* si, double* a) {
  if (src < 1 || dst < 1 || dst > src || !n || !si || !a) return fail(JDS_EINVAL, "bad argument");
  AreaTap* t = (AreaTap*)malloc(sizeof(AreaTap) * (size_t)dst);
  if (!t) return fail(JDS_ENOMEM, "host allocation failed");
  if (area_tab_build(src, dst, t) < 0) {
    free(t);
    return fail(JDS_EINVAL, "more than 4 taps per sample");
  }
  for (int d = 0; d < dst; ++d) {
    n[d] = t[d].n;
    for (int k = 0; k < 4; ++k) {
      si[4 * d + k] = k < t[d].n ? t[d].si[k] : -1;
      a[4 * d + k] = k < t[d].n ? t[d].a[k] : 0.0;
    }
  }
  free(t);
  return JDS_OK;
}

int jds_selftest_dct16x16(const double* in, double* out, int64_t n, int32_t inverse) {
  if (!in || !out || n < 0) return fail(JDS_EINVAL, "bad argument");
  for (int64_t b = 0; b < n; ++b) {
    double t[256], c[16];
    memcpy(t, in + 256 * b, sizeof t);
    for (int col = 0; col < 16; ++col) {  // axis 0 first
      for (int i = 0; i < 16; ++i) c[i] = t[i * 16 + col];
      if (inverse) dct3_line16(c); else dct2_line16(c);
      for (int i = 0; i < 16; ++i) t[i * 16 + col] = c[i];
    }
    for (int r = 0; r < 16; ++r) {
      if (inverse) dct3_line16(t + 16 * r); else dct2_line16(t + 16 * r);
    }
    for (int i = 0; i < 256; ++i) out[256 * b + i] = t[i] * 0.03125;  // pocketfft fct = 1/32
  }
  return JDS_OK;
}

}  // extern "C"
