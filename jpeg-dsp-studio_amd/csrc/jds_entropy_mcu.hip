// jds_entropy_mcu.hip — the interleaved-scan writer (DESIGN.md "Transcode";
// byte-for-byte definition: tests/transcode_ref.py).  jds_entropy.hip writes
// this library's own profile: three non-interleaved scans of frames of one plan
// geometry.  This unit writes the form everybody else reads and writes -- ONE
// scan of Ns = 3 in MCU order -- for a batch of files of any sizes and modes,
// straight from the planar coefficients of jds_decode_jpeg (no re-ordering
// pass), with the Annex K tables or each file's own optimised ones.  It is the
// one-pass coder again (jds_entropy_core.hpp: es_block, es_place, em_copy), with
//   * segments of 64 consecutive blocks of the scan IN SCAN ORDER: a lane maps
//     its scan position to (MCU, slot), component, block row and column of the
//     component's T.81 grid, or to "padding" (mcu_locate);
//   * the DC predecessor by index arithmetic (mcu_pred), not the neighbouring
//     lane: segment boundaries do not align with MCUs;
//   * padding blocks coded as libjpeg's dummy blocks: zero DC difference, EOB;
//   * per-file geometry records (McuFile) and a segment table over all files
//     (segfile) where the three-scan writer has one EntGeo per batch.
// Launches per batch: [memset, k_mcu_hist, k_ent_opt_tables] k_mcu_walk
// [k_mcu_fscan<0>: files with more than ES_SELF_MAX segments] k_mcu_place
// k_mcu_fscan<1>; the host reads the files' lengths and flags once and places
// the files; k_mcu_head, k_mcu_emit.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_entropy_common.hpp"
#include "jds_entropy_core.hpp"
#include "jds_entropy_mcu.hpp"
#include "jds_entropy_mcu_dev.hpp"
#include "jds_internal.hpp"

namespace jds {

// a wave's file record, read in place: the index is wave-uniform, so its fields
// arrive by scalar loads (a by-value copy of the record went to scratch memory,
// 120 B per lane, in the two kernels that walk it)
__device__ __forceinline__ const McuFile& mcu_file(const McuFile* __restrict__ files,
                                                   const int32_t* __restrict__ segfile, int g) {
  return files[__builtin_amdgcn_readfirstlane(segfile[g])];
}

// ---------------------------------------------------------- histogram --

constexpr int MH_WAVES = 4;
// copies of a wave's bins (k_ent_hist's EH_COPIES; here a wave counts both
// classes, so half as many fit the same LDS)
constexpr int MH_COPIES = 4;

// k_ent_hist's counts over the interleaved scan: one wave per segment, both
// classes per wave (a segment holds luma and chroma blocks), a padding block's
// two symbols (DC category 0, EOB) with the others.
__global__ void __launch_bounds__(64 * MH_WAVES) k_mcu_hist(const McuFile* __restrict__ files,
                                                            const int32_t* __restrict__ segfile, const int nseg,
                                                            const int16_t* __restrict__ coeffs,
                                                            OptFrame* __restrict__ of) {
  __shared__ uint32_t bins_s[MH_WAVES][2][OPT_BINS * MH_COPIES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = lane; i < 2 * OPT_BINS * MH_COPIES; i += 64) (&bins_s[wv][0][0])[i] = 0u;
  __syncthreads();
  const int g = blockIdx.x * MH_WAVES + wv;
  if (g >= nseg) return;  // (whole wave; no workgroup barrier follows)
  const McuFile& F = mcu_file(files, segfile, g);
  const int n = (g - F.seg0) * 64 + lane;
  if (n < F.nblk) {
    long long a;
    const McuPos pos = mcu_pos(F, n);
    const int c = mcu_locate(F, pos, a);
    uint32_t* bins = bins_s[wv][c ? 1 : 0] + (lane & (MH_COPIES - 1));
    if (a >= 0) {
      const BlockRegs rg = load_block(coeffs + a);
      const long long pa = mcu_pred(F, pos);
      const int diff = coef_at<0>(rg) - (pa >= 0 ? (int)coeffs[pa] : 0);
      const int da = diff < 0 ? -diff : diff;
      int ds = da ? 32 - __clz(da) : 0;
      ds = ds > 11 ? 11 : ds;
      atomicAdd(&bins[ds * MH_COPIES], 1u);
      int aor = 0, last = 0;
      eh_ac<1, MH_COPIES>(rg, 0, aor, bins, last);
      if (last < 63) atomicAdd(&bins[EH_EOB * MH_COPIES], 1u);
    } else {
      atomicAdd(&bins[0], 1u);
      atomicAdd(&bins[EH_EOB * MH_COPIES], 1u);
    }
  }
  __builtin_amdgcn_wave_barrier();  // one wave: its LDS operations execute in order
  asm volatile("" ::: "memory");
  for (int cls = 0; cls < 2; ++cls) {
    uint32_t* cnt = of[F.frame].cnt[cls];
    for (int i = lane; i < OPT_BINS; i += 64) {
      uint32_t v = 0u;
#pragma unroll
      for (int k = 0; k < MH_COPIES; ++k) v += bins_s[wv][cls][i * MH_COPIES + k];
      if (v) atomicAdd(&cnt[i], v);
    }
  }
}

// --------------------------------------------------------------- walk --

// k_ent_walk over scan-order segments.  Every wave stages its own file's code
// table (a workgroup's segments can lie in different files).
__global__ void __launch_bounds__(64 * ES_WAVES) __attribute__((amdgpu_waves_per_eu(ES_WPE))) k_mcu_walk(
    const McuFile* __restrict__ files, const int32_t* __restrict__ segfile, const int nseg,
    const int16_t* __restrict__ coeffs, uint32_t* __restrict__ gst, uint32_t* __restrict__ nbits,
    unsigned long long* __restrict__ agg, uint32_t* __restrict__ badseg, const OptFrame* __restrict__ of) {
  __shared__ EsTab es_s[ES_WAVES];
  __shared__ uint32_t stage[ES_WAVES][ES_SW > 0 ? ES_SW : 1][64];
  __shared__ int16_t czs[ES_WAVES][ES_HI > 0 ? ES_HI : 1][64];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  int16_t* cz = &czs[wv][0][lane];
  const int g = blockIdx.x * ES_WAVES + wv;
  const McuFile& F = mcu_file(files, segfile, g < nseg ? g : nseg - 1);
  {
    const uint32_t* src = reinterpret_cast<const uint32_t*>(&of[F.frame].es);
    uint32_t* dst = reinterpret_cast<uint32_t*>(&es_s[wv]);
    for (int i = lane; i < (int)(sizeof(EsTab) / 4); i += 64) dst[i] = src[i];
    __syncthreads();
  }
  const EsTab& es = es_s[wv];
  if (g >= nseg) return;  // (whole wave; no barrier follows)
  const int n = (g - F.seg0) * 64 + lane;
  const bool valid = n < F.nblk;
  long long a = -1ll;
  int c = 0, pred = 0;
  BlockRegs rg;
#pragma unroll
  for (int i = 0; i < 32; ++i) rg.w[i] = 0u;
  if (valid) {
    const McuPos pos = mcu_pos(F, n);
    c = mcu_locate(F, pos, a);
    if (a >= 0) {
      rg = load_block(coeffs + a);
      const long long pa = mcu_pred(F, pos);
      pred = pa >= 0 ? (int)coeffs[pa] : 0;
    }
  }
  // a padding block: all zero, DC difference 0
  const int diff = a >= 0 ? coef_at<0>(rg) - pred : 0;
  uint32_t* st = &stage[wv][0][lane];
  uint32_t* ov = gst + (size_t)g * ES_MAXW * 64 + lane;
  uint32_t nb = 0u;
  int k = 0;
  bool bd = false;
  if (valid) {
    EsStage o{st, ov};
    nb = es_block(rg, diff, es, c ? 1 : 0, o, bd, cz);
    k = (int)((nb + 31u) >> 5);
  }
  const bool any_bad = __ballot(bd) != 0ull;
  // the LDS slots to the segment's global area (one 256-B row per slot)
  const int kmax = (int)wave_max((uint32_t)(k < ES_SW ? k : ES_SW));
  for (int j = 0; j < kmax; ++j)
    if (j < k) ov[j * 64] = st[j * 64];
  nbits[(size_t)g * 64 + lane] = nb;
  const unsigned long long t = wave_sum(nb);  // (<= 64 * 1665 bits)
  if (lane == 0) {
    agg[g] = t;
    badseg[g] = any_bad ? 1u : 0u;
  }
}

// ---------------------------------------------------------- placement --

// k_ent_place with the file for the scan: incl[g] = the segment's end bit
// within its file's scan, fbits[file] = the scan's bits.
__global__ void __launch_bounds__(256) k_mcu_place(const McuFile* __restrict__ files,
                                                   const int32_t* __restrict__ segfile, const int nseg,
                                                   const uint32_t* __restrict__ gst,
                                                   const uint32_t* __restrict__ nbits,
                                                   const unsigned long long* __restrict__ agg,
                                                   const unsigned long long* __restrict__ segoff,
                                                   unsigned long long* __restrict__ incl, uint32_t* __restrict__ raw,
                                                   unsigned long long* __restrict__ ffs,
                                                   unsigned long long* __restrict__ fbits) {
  const int lane = threadIdx.x & 63;
  const int g = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (g >= nseg) return;
  const int fi = __builtin_amdgcn_readfirstlane(segfile[g]);
  const McuFile F = files[fi];
  const int seg = g - F.seg0;
  const bool valid = seg * 64 + lane < F.nblk;
  const int nvalid = F.nblk - seg * 64 < 64 ? F.nblk - seg * 64 : 64;
  const bool last_seg = seg == F.nseg - 1;
  const bool fuse = !last_seg;      // this segment completes the word it shares with the next
  const int gn = fuse ? g + 1 : g;  // the next segment of the scan (its head bits)
  const uint32_t nb = nbits[(size_t)g * 64 + lane];
  const uint32_t nbn = nbits[(size_t)gn * 64 + lane];
  const uint32_t w0n = gst[(size_t)gn * ES_MAXW * 64 + lane];  // (row 0; garbage where nbn == 0)
  unsigned long long pre;
  if (F.nseg <= ES_SELF_MAX) {  // (uniform: the scan's length)
    const unsigned long long* a0 = agg + F.seg0;
    uint32_t ps = 0u;
    for (int j0 = 0; j0 < seg; j0 += 512) {  // eight loads in flight per lane
      uint32_t t[8];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const int j = j0 + 64 * u + lane;
        t[u] = j < seg ? (uint32_t)a0[j] : 0u;
      }
#pragma unroll
      for (int u = 0; u < 8; ++u) ps += t[u];
    }
    pre = ((unsigned long long)wave_sum(ps >> 8) << 8) + wave_sum(ps & 255u);
  } else {
    pre = segoff[g];  // (file-relative prefixes, k_mcu_fscan<false>)
  }
  const uint32_t inc = wave_incl_sum(nb, lane), incn = wave_incl_sum(nbn, lane);
  const unsigned long long A = lane63(inc);
  const unsigned long long W1 = pre + A;
  if (lane == 0) {
    incl[g] = W1;
    if (last_seg) fbits[fi] = W1;
  }
  uint32_t tailx = 0u;
  unsigned long long Wn = 0ull;
  if (fuse) {
    // the next segment's lanes starting inside this segment's final word: each
    // one's bits there are its first staged word's leading bits
    const uint32_t sh = (uint32_t)(W1 & 31ull), p = sh + (incn - nbn);
    tailx = (sh && nbn && p < 32u) ? w0n >> p : 0u;
    tailx = wave_or(tailx);
    const unsigned long long An = lane63(incn);
    if (seg + 2 == F.nseg && sh && ((W1 + An - 1ull) >> 5) == ((W1 - 1ull) >> 5)) Wn = W1 + An;
  }
  // (a block costs >= 2 bits with any table, padding blocks included: the optimised route's span)
  const EntGeo e{};
  const EsSeg q{};
  es_place<es_span<true>()>(e, q, g, lane, valid, nvalid, last_seg, nb, inc - nb, pre, A, nullptr,
                            gst + (size_t)g * ES_MAXW * 64 + lane, (int)((nb + 31u) >> 5), raw, ffs, nullptr, nullptr,
                            fuse, tailx, Wn, raw + F.raw_w0, false);
}

// ------------------------------------------------- per-file prefixes --

// the bytes of a frame's DHT segments that a file carries: all four, or for a
// grayscale file the first two (DC 0x00, AC 0x10: the luma class leads the
// frame's header), found by the segments' own length fields
__device__ __forceinline__ int mcu_dht_len(const McuFile& F, const OptFrame& o) {
  if (!F.gray) return (int)o.hdr_len - ENT_HDR_FIXED;
  const uint8_t* h = o.hdr + ENT_HDR_FIXED;
  const int l0 = 2 + ((h[2] << 8) | h[3]);
  return l0 + 2 + ((h[l0 + 2] << 8) | h[l0 + 3]);
}

// the file's bytes before its scan: SOI, prefix, its DHT segments, SOS
__device__ __forceinline__ long long mcu_head_len(const McuFile& F, const OptFrame* __restrict__ of) {
  return 2ll + F.pfx_len + mcu_dht_len(F, of[F.frame]) + (F.gray ? MCU_SOS1 : MCU_SOS);
}

// k_ent_fscan per file (one 1024-thread workgroup each): out[g] = the
// file-relative exclusive prefix of in[g] over the file's segments.  OFFS (in =
// the segments' 0xFF counts): also every segment's first output byte within its
// file, the file's length and its "not baseline-codable" flag.
template <bool OFFS>
__global__ void __launch_bounds__(1024) k_mcu_fscan(const McuFile* __restrict__ files,
                                                    const unsigned long long* __restrict__ in,
                                                    unsigned long long* __restrict__ out,
                                                    const unsigned long long* __restrict__ desc,
                                                    const unsigned long long* __restrict__ fbits,
                                                    unsigned long long* __restrict__ outoff,
                                                    const uint32_t* __restrict__ badseg,
                                                    const OptFrame* __restrict__ of,
                                                    unsigned long long* __restrict__ flen,
                                                    uint32_t* __restrict__ fbad) {
  __shared__ unsigned long long s_w[16];
  __shared__ int s_bad;
  const int f = blockIdx.x, t = threadIdx.x, lane = t & 63, wv = t >> 6;
  const McuFile F = files[f];
  const int n = F.nseg;
  if (!OFFS && n <= ES_SELF_MAX) return;  // (whole workgroup: k_mcu_place sums such a file's totals itself)
  const long long g0 = F.seg0;
  const int C = (n + 1023) / 1024, i0 = min(n, t * C), i1 = min(n, i0 + C);
  if (t == 0) s_bad = 0;
  unsigned long long loc = 0ull;
  for (int i = i0; i < i1; ++i) loc += in[g0 + i];
  unsigned long long inc = loc;
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const unsigned long long y = __shfl_up(inc, o, 64);
    if (lane >= o) inc += y;
  }
  if (lane == 63) s_w[wv] = inc;
  __syncthreads();
  unsigned long long base = 0ull, all = 0ull;
  for (int w = 0; w < 16; ++w) {
    base += w < wv ? s_w[w] : 0ull;
    all += s_w[w];
  }
  unsigned long long run = base + inc - loc;
  const long long hl = OFFS ? mcu_head_len(F, of) : 0ll;
  int b = 0;
  for (int i = i0; i < i1; ++i) {
    const unsigned long long v = in[g0 + i];
    out[g0 + i] = run;
    if constexpr (OFFS) {
      const unsigned long long W0 = i ? desc[g0 + i - 1] : 0ull;
      outoff[g0 + i] = (unsigned long long)hl + 4 * ((W0 + 31) >> 5) + run;
      b |= (int)badseg[g0 + i];
    }
    run += v;
  }
  if constexpr (OFFS) {
    if (b) s_bad = 1;
    __syncthreads();
    if (t == 0) {
      flen[f] = (unsigned long long)hl + ((fbits[f] + 7) >> 3) + all + 2ull;
      fbad[f] = (uint32_t)s_bad;
    }
  }
}

// --------------------------------------------------------------- emit --

// A file's bytes around its scan: SOI, the prefix, the DHT segments of its
// tables, SOS, EOI.  fout[f] < 0: the file is not written.
__global__ void __launch_bounds__(256) k_mcu_head(const McuFile* __restrict__ files, const uint8_t* __restrict__ pfx,
                                                  const OptFrame* __restrict__ of,
                                                  const unsigned long long* __restrict__ flen,
                                                  const long long* __restrict__ fout, uint8_t* __restrict__ out) {
  const int f = blockIdx.x, t = threadIdx.x;
  if (fout[f] < 0) return;
  const McuFile F = files[f];
  uint8_t* dst = out + fout[f];
  const OptFrame& o = of[F.frame];
  const int nd = mcu_dht_len(F, o);
  if (t == 0) {
    dst[0] = 0xFF;
    dst[1] = 0xD8;
  }
  const uint8_t* ps = pfx + F.pfx_off;
  for (int i = t; i < F.pfx_len; i += 256) dst[2 + i] = ps[i];
  uint8_t* d2 = dst + 2 + F.pfx_len;
  for (int i = t; i < nd; i += 256) d2[i] = o.hdr[ENT_HDR_FIXED + i];
  if (F.gray) {  // (uniform: a field of the file's record)
    if (t < MCU_SOS1) {
      const uint8_t sos[MCU_SOS1] = {0xFF, 0xDA, 0x00, 0x08, 0x01, (uint8_t)F.comp_id, 0x00, 0x00, 0x3F, 0x00};
      d2[nd + t] = sos[t];
    }
  } else if (t < MCU_SOS) {
    const uint8_t sos[MCU_SOS] = {0xFF, 0xDA, 0x00, 0x0C, 0x03, 1, 0x00, 2, 0x11, 3, 0x11, 0x00, 0x3F, 0x00};
    d2[nd + t] = sos[t];
  }
  if (t == 0) {
    const unsigned long long len = flen[f];
    dst[len - 2] = 0xFF;
    dst[len - 1] = 0xD9;
  }
}

// k_ent_emit3 per file: one wave per segment, the stuffed bytes of the words it finalised
__global__ void __launch_bounds__(256) k_mcu_emit(const McuFile* __restrict__ files,
                                                  const int32_t* __restrict__ segfile, const int nseg,
                                                  const unsigned long long* __restrict__ desc,
                                                  const unsigned long long* __restrict__ fbits,
                                                  const uint32_t* __restrict__ raw,
                                                  const unsigned long long* __restrict__ outoff,
                                                  const long long* __restrict__ fout, uint8_t* __restrict__ out) {
  __shared__ uint32_t sbuf[4][(2 * EM_CHUNK + 8) / 4];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int g = blockIdx.x * 4 + wv;
  if (g >= nseg) return;
  const int fi = __builtin_amdgcn_readfirstlane(segfile[g]);
  const long long fo = fout[fi];
  if (fo < 0) return;
  const McuFile F = files[fi];
  const int seg = g - F.seg0;
  const unsigned long long W0 = seg ? desc[g - 1] : 0ull, W1 = desc[g];
  const unsigned long long nbytes = (fbits[fi] + 7) >> 3;
  const unsigned long long fw = (W0 + 31) >> 5, lw = (W1 - 1) >> 5;
  if (fw > lw) return;
  const unsigned long long b0 = 4 * fw, b1 = (4 * lw + 4 < nbytes) ? 4 * lw + 4 : nbytes;
  em_copy(raw + F.raw_w0, b0, b1, out + fo + (long long)outoff[g], sbuf[wv], lane);
}

// ------------------------------------------------------------ driver --

long long mcu_raw_words(int nblk) { return ((long long)nblk * ENT_BLOCK_BITS_OPT + 31) / 32 + 2; }

// worst case file: SOI, prefix, four full DHT segments, SOS, every block at
// its bound with all bytes stuffed, EOI
long long mcu_capacity(const McuFile& f) {
  return 2ll + f.pfx_len + (ENT_HDR - ENT_HDR_FIXED) + MCU_SOS + 2 * 4 * f.raw_words + 2;
}

size_t mcu_scratch_bytes(int nf, long long nseg, long long raw_words) {
  McuDev d;
  return mcu_carve(nullptr, nf, nseg, raw_words, &d);
}

size_t mcu_carve(void* base, int nf, long long nseg, long long raw_words, McuDev* d) {
  size_t o = 0;
  auto take = [&](size_t bytes) {
    void* p = base ? (char*)base + o : nullptr;
    o = (o + bytes + 255) & ~(size_t)255;
    return p;
  };
  const size_t ns = (size_t)nseg, f = (size_t)nf;
  d->desc = (unsigned long long*)take(8 * (ns + 1));
  d->agg = (unsigned long long*)take(8 * (ns + 1));
  d->segoff = (unsigned long long*)take(8 * (ns + 1));
  d->ffs = (unsigned long long*)take(8 * (ns + 1));
  d->ffx = (unsigned long long*)take(8 * (ns + 1));
  d->outoff = (unsigned long long*)take(8 * (ns + 1));
  d->nbits = (uint32_t*)take(4 * 64 * ns);
  d->badseg = (uint32_t*)take(4 * (ns + 1));
  d->fbits = (unsigned long long*)take(8 * f);
  d->flen = (unsigned long long*)take(8 * f);
  d->fbad = (uint32_t*)take(4 * f);
  d->fout = (long long*)take(8 * f);
  d->of = (OptFrame*)take(sizeof(OptFrame) * (f + 1));
  d->hdr_std = (uint8_t*)take(ENT_HDR);
  d->raw = (uint32_t*)take(4 * (size_t)raw_words);
  d->gst = (uint32_t*)take(4 * (size_t)ES_MAXW * 64 * ns);
  return o;
}

size_t mcu_optframe_bytes() { return sizeof(OptFrame); }

// the shared Annex K frame (optimize = 0): the standard symbols and DHT segments
void mcu_std_frame(const EsTab* es_host, const uint8_t* hdr_std, void* out) {
  OptFrame* o = (OptFrame*)out;
  memset(o, 0, sizeof *o);
  o->es = *es_host;
  o->hdr_len = ENT_HDR;
  memcpy(o->hdr, hdr_std, ENT_HDR);
}

// Everything up to the files' lengths: d.flen / d.fbad are final when the
// stream reaches the end of these launches.  optimize: d.of[0 .. nf) are the
// files' own frames (built here from their counts); otherwise d.of[0] is the
// caller's Annex K frame (mcu_std_frame).
hipError_t launch_mcu_code(const McuDev& d, int nf, int nseg, bool any_long, const int16_t* coeffs, bool optimize,
                           const EsTab* std_tab, hipStream_t s) {
  hipError_t err;
  if (optimize) {
    if ((err = hipMemsetAsync(d.of, 0, sizeof(OptFrame) * (size_t)nf, s)) != hipSuccess) return err;
    hipLaunchKernelGGL(k_mcu_hist, dim3((nseg + MH_WAVES - 1) / MH_WAVES), dim3(64 * MH_WAVES), 0, s, d.files,
                       d.segfile, nseg, coeffs, d.of);
    kmark(s, "k_mcu_hist");
    if ((err = hipGetLastError()) != hipSuccess) return err;
    if ((err = launch_opt_tables(nf, std_tab, d.hdr_std, 0ll, d.of, s)) != hipSuccess) return err;
  }
  hipLaunchKernelGGL(k_mcu_walk, dim3((nseg + ES_WAVES - 1) / ES_WAVES), dim3(64 * ES_WAVES), 0, s, d.files, d.segfile,
                     nseg, coeffs, d.gst, d.nbits, d.agg, d.badseg, d.of);
  kmark(s, "k_mcu_walk");
  if ((err = hipGetLastError()) != hipSuccess) return err;
  if (any_long) {
    hipLaunchKernelGGL(k_mcu_fscan<false>, dim3(nf), dim3(1024), 0, s, d.files, d.agg, d.segoff, nullptr, nullptr,
                       nullptr, nullptr, nullptr, nullptr, nullptr);
    kmark(s, "k_mcu_fscan<0>");
  }
  hipLaunchKernelGGL(k_mcu_place, dim3((nseg + 3) / 4), dim3(256), 0, s, d.files, d.segfile, nseg, d.gst, d.nbits,
                     d.agg, d.segoff, d.desc, d.raw, d.ffs, d.fbits);
  kmark(s, "k_mcu_place");
  if ((err = hipGetLastError()) != hipSuccess) return err;
  hipLaunchKernelGGL(k_mcu_fscan<true>, dim3(nf), dim3(1024), 0, s, d.files, d.ffs, d.ffx, d.desc, d.fbits, d.outoff,
                     d.badseg, d.of, d.flen, d.fbad);
  kmark(s, "k_mcu_fscan<1>");
  return hipGetLastError();
}

// The files at d.fout (uploaded by the caller; < 0: not written) into out.
hipError_t launch_mcu_emit(const McuDev& d, int nf, int nseg, uint8_t* out, hipStream_t s) {
  hipLaunchKernelGGL(k_mcu_head, dim3(nf), dim3(256), 0, s, d.files, d.pfx, d.of, d.flen, d.fout, out);
  kmark(s, "k_mcu_head");
  hipLaunchKernelGGL(k_mcu_emit, dim3((nseg + 3) / 4), dim3(256), 0, s, d.files, d.segfile, nseg, d.desc, d.fbits,
                     d.raw, d.outoff, d.fout, out);
  kmark(s, "k_mcu_emit");
  return hipGetLastError();
}

int mcu_self_max() { return ES_SELF_MAX; }

}  // namespace jds
