// jds_abi.hpp — what the units of the C-ABI share (jds_abi.hip: contexts, plans,
// the codec's host path; jds_abi_jpeg.hip: foreign files): the error slot, the
// context, and the launchers' prototypes of the kernel units.  Private to csrc/.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>
#include <stdarg.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <cmath>
#include <thread>
#include <vector>

#include "jds_huffdec.hpp"
#include "jds_huffopt.hpp"
#include "jds_internal.hpp"
#include "jds_jpeg_inv.hpp"

namespace jds {
hipError_t launch_codec(int mode, bool pf, const Geo& g, int n, const uint8_t* rgb, uint8_t* rgb_out,
                        int16_t* coeffs, const FrameQ* fq, const double* gk, jds_frame_stats* st,
                        double* part, bool want_sse, double* err_y, double* err_rgb, jds_selected_block* sel,
                        int sel_blk, hipStream_t s, hipEvent_t* ev, int phases, int in_div, const GenBufs* gb,
                        const InvFix* fx = nullptr);
int inv_tiles(int mode, int H, int W);
void inv_rows(int mode, int H, int ty, int* out);
int inv_rows_need(int mode, int H, int ty, int by, int r);
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
void inv_cert_forms_host(const double* v, long long n, uint8_t* bytes, uint8_t* certain, double* consts);
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
// the scaled libjpeg rendering (jds_jpeg_ljs.hip): denom 2, 4 or 8; the batch's arrays are per mode and denominator index
hipError_t launch_jpeg_ljs(const JInvArgs& a, int denom, const int16_t* coeffs, uint8_t* rgb, hipStream_t s);
hipError_t launch_jpeg_ljs_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES][3],
                                 const int nmap[JI_MODES][3], const int tiles[JI_MODES][3], const uint32_t* status,
                                 const int16_t* coeffs, uint8_t* rgb, hipStream_t s);
// Pillow resizing (jds_resize.hip; records and maps: jds_resize.hpp)
struct RsRec;
struct RsMap;
hipError_t launch_resize(const RsRec& r, const int32_t* tabs, const uint8_t* src, uint8_t* dst, hipStream_t s);
hipError_t launch_resize_batch(const RsRec* recs, const RsMap* map, int nmap, int tiles, const uint32_t* status,
                               const int32_t* tabs, const uint8_t* src0, const uint8_t* src1, uint8_t* dst0,
                               uint8_t* dst1, hipStream_t s);
hipError_t launch_jpeg_fwd(const JInvArgs& a, const uint8_t* img, int16_t* coeffs, hipStream_t s);
hipError_t launch_jpeg_fwd_batch(const JInvRec* recs, const JInvMap* maps, const int map_off[JI_MODES],
                                 const int nmap[JI_MODES], const int tiles[JI_MODES], const uint8_t* img,
                                 int16_t* coeffs, hipStream_t s);
}

using namespace jds;

extern thread_local char g_err[512];  // jds_last_error (defined in jds_abi.hip)

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
  // foreign files (batch_run, jds_abi_jpeg.hip; a single-file call is a batch of one): the decode kernels'
  // scratch and the DC staging array of the interleaved scans; everything a run uploads (file bytes, table
  // sets, MCU and inverse records, tile maps, interval lists, initial status words) is gathered in one
  // pinned host buffer and copied once to bat
  DevBuf dec_scr, dec_mcu;
  DevBuf bat;
  DevBuf mcu_up, mcu_scr;  // interleaved-scan writer (jds_jpeg_transcode): its uploads (records, segment table, prefixes), scratch
  void* bat_host = nullptr;
  size_t bat_host_cap = 0;
  // Pillow resizing: the tables, records and maps of a call (pinned host staging, device copy), the scratch
  // image of the tall-image rule, jds_jpeg_batch_to_tensor's decoded images, the event behind a call's launches
  DevBuf rsz_tab, rsz_tall, rsz_src;
  void* rsz_host = nullptr;
  size_t rsz_host_cap = 0;
  hipEvent_t rsz_ev = nullptr;
  // jds_ctx_profile: launch marks of the batch calls on this context
  KMarks marks;
  bool prof_on = false;
  DevBuf gen_tab, gen_sub, gen_rec;  // general-geometry path (jds_gen.hip)
  // progressive files on a profiled context (jds_pjpeg_scan_times): the walk time of every scan
  // of the last batch, in chain order (device ticks, then microseconds)
  DevBuf pj_ticks;
  std::vector<double> pj_scan_us;
  size_t ss_budget = 0;  // SSIM scratch budget per launch group (0: SSIM_SCRATCH; jds_ctx_set_ssim_scratch)
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

// The prefilter's column pass is cv2's SymmColumnFilter, k1 T[y] + k0 (T[y+1] +
// T[y-1]) (engines/color_space.py:39-40 through sepFilter2D): defined for
// symmetric taps only, which is all cv2 hands it.  The exact kernels restate
// that form, the certified kernels weigh rows by k0, k0+k1, k1+k2, k2; the two
// agree only when gauss[0] == gauss[2].  Taps are read only where the
// prefilter runs (prefilter != 0 and not 4:4:4).
static int check_taps(const double* gauss, int subsampling, int prefilter) {
  if (!prefilter || subsampling == JDS_SS_444) return JDS_OK;
  if (!std::isfinite(gauss[0]) || !std::isfinite(gauss[1]) || !std::isfinite(gauss[2]) || gauss[0] != gauss[2])
    return fail(JDS_EINVAL,
                "prefilter taps [%.17g, %.17g, %.17g] must be finite and symmetric (gauss[0] == gauss[2]): the column "
                "pass is cv2's symmetric filter",
                gauss[0], gauss[1], gauss[2]);
  return JDS_OK;
}

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

// c->ent_cf (a decoded frame) -> rgb_out by the plan's inverse (jds_abi.hip).
int inverse_of_decoded(jds_ctx* c, const jds_params* prm, int64_t H, int64_t W, int64_t n_coeffs, uint8_t* rgb_out,
                       int16_t* coeffs);

// A batch resize (jds_abi_resize.hip): image i of n is H x W at byte `off` of
// the source, its slot bytes [i, i + 1) * oh * ow * 3 of the output; st: the
// status word that zeroes the slot when set (-1: none), zero: the slot is zeros.
struct ResizeSrc {
  long long off, H, W;
  int st, zero, has_box;
  float box[4];
};
struct ResizeJob;
// The plans, tables and records on the host (JDS_EINVAL / JDS_ENOTSUP as jds.h says).
int resize_job_build(const ResizeSrc* items, int n, long long oh, long long ow, int resample, ResizeJob** out);
// The upload and the launches on s; wait: return once they have run (the staging and the tables may be
// rewritten); without it the caller synchronises s before the context is used again.
int resize_job_enqueue(jds_ctx* c, ResizeJob* j, const uint8_t* src_dev, const uint32_t* status_dev, uint8_t* out_dev,
                       hipStream_t s, bool wait);
void resize_job_free(ResizeJob* j);
void resize_ctx_release(jds_ctx* c);
