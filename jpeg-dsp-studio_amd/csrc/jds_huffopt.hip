// jds_huffopt.hip — the front of the optimised-table entropy route (DESIGN.md
// "Optimised tables"; definition: tests/huffopt_ref.py).  The writer's standard
// route codes every frame with the T.81 Annex K tables; this one gives each
// frame its own four tables, built on the device so that jds_plan_entropy_opt
// stays asynchronous:
//   k_ent_hist        the symbol counts of every frame: one wave per 64-block
//                     segment (the coder's geometry and DC predecessor rule),
//                     one lane per block, LDS atomics into the wave's bins,
//                     the non-zero bins flushed with global integer atomics
//                     into the frame's [2 classes][16 + 256] counters (integer
//                     sums: the result does not depend on the order).
//   k_ent_opt_tables  one wave per table, four tables per frame: T.81 K.2 with
//                     libjpeg's tie rules (jds_huffopt.hpp), K.3, the frame's
//                     left-aligned code table, its four DHT segments and its
//                     header length.
// The coding kernels (jds_entropy.hip, OPT = true) then read each frame's
// OptFrame.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_entropy_common.hpp"
#include "jds_entropy_core.hpp"
#include "jds_huffopt.hpp"
#include "jds_internal.hpp"

namespace jds {

// ---------------------------------------------------------- histogram --

constexpr int EH_WAVES = 4;
// Copies of a wave's bins, lane l counting into copy l % EH_COPIES (bin i's
// copies side by side, on neighbouring banks): the lanes of a wave mostly count
// the same few symbols, and LDS atomics on one address take their turns
// (1 copy: 0.187, 8 copies: 0.143 ms per 64 x 1080p Q50).
constexpr int EH_COPIES = 8;
static_assert(EH_COPIES >= 1 && (EH_COPIES & (EH_COPIES - 1)) == 0 && EH_COPIES <= 64, "a power of two");

// RST: every segment is a restart interval (its first block predicts from 0).
// A block baseline JPEG cannot code (DC category > 11, AC category > 10) counts
// with the coder's clamps; the coding kernels report its frame (lengths = 0).
template <bool RST>
__global__ void __launch_bounds__(64 * EH_WAVES) k_ent_hist(const EntGeo e, const int nseg,
                                                            const int16_t* __restrict__ coeffs,
                                                            OptFrame* __restrict__ of) {
  __shared__ uint32_t bins_s[EH_WAVES][OPT_BINS * EH_COPIES];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  for (int i = lane; i < OPT_BINS * EH_COPIES; i += 64) bins_s[wv][i] = 0u;
  uint32_t* bins = bins_s[wv] + (lane & (EH_COPIES - 1));  // the lane's copy: bin i at bins[i * EH_COPIES]
  __syncthreads();
  const int g = blockIdx.x * EH_WAVES + wv;
  const bool active = g < nseg;  // (whole wave)
  const EsSeg q = es_seg(e, active ? g : nseg - 1);
  if (active) {
    const int bi = q.seg * 64 + lane;
    const bool valid = bi < q.nbs;
    const long long gb = (long long)q.f * e.nb + e.first[q.s] + (valid ? bi : q.nbs - 1);
    const BlockRegs rg = load_block(coeffs + gb * 64);
    const int dc = coef_at<0>(rg);
    int pred = wave_shr1(dc);
    if (lane == 0) pred = (!RST && q.seg) ? (int)coeffs[(gb - 1) * 64] : 0;
    if (valid) {
      const int diff = dc - pred;
      const int da = diff < 0 ? -diff : diff;
      int ds = da ? 32 - __clz(da) : 0;
      ds = ds > 11 ? 11 : ds;
      atomicAdd(&bins[ds * EH_COPIES], 1u);
      int aor = 0, last = 0;
      eh_ac<1, EH_COPIES>(rg, 0, aor, bins, last);
      if (last < 63) atomicAdd(&bins[EH_EOB * EH_COPIES], 1u);
    }
  }
  __syncthreads();
  if (active) {
    uint32_t* cnt = of[q.f].cnt[q.s ? 1 : 0];
    for (int i = lane; i < OPT_BINS; i += 64) {
      uint32_t v = 0u;
#pragma unroll
      for (int c = 0; c < EH_COPIES; ++c) v += bins_s[wv][i * EH_COPIES + c];
      if (v) atomicAdd(&cnt[i], v);
    }
  }
}

hipError_t launch_ent_hist(const EntGeo& e, int nseg, const int16_t* coeffs, bool rst, OptFrame* of, hipStream_t s) {
  if ((long long)e.nb * 64 >= (1ll << 32)) return hipErrorInvalidValue;  // a table's counts stay below 2^32
  const unsigned wg = (unsigned)((nseg + EH_WAVES - 1) / EH_WAVES);
  if (rst)
    hipLaunchKernelGGL(k_ent_hist<true>, dim3(wg), dim3(64 * EH_WAVES), 0, s, e, nseg, coeffs, of);
  else
    hipLaunchKernelGGL(k_ent_hist<false>, dim3(wg), dim3(64 * EH_WAVES), 0, s, e, nseg, coeffs, of);
  kmark(s, "k_ent_hist");
  return hipGetLastError();
}

// ------------------------------------------------------- table builder --

constexpr int OT_WAVES = 4;  // a frame's four tables: DC luma, AC luma, DC chroma, AC chroma (the DHT order)

struct OtWave {
  uint16_t parent[HO_NODES];    // merge tree: 0xFFFF = root / unused
  uint16_t node[HO_SYMS + 1];   // live entry -> its current tree node
  uint32_t bits[33];            // codes per length; after ho_limit only 1..16
  uint32_t base[33];            // counted symbols per size, then each size's first HUFFVAL position
  uint32_t first[18], cum[18];  // ho_starts
  uint32_t code[256];           // symbol -> length << 16 | code
  uint8_t dht[(ENT_DHT_HEAD + 256 + 3) / 4 * 4];  // the DHT segment: FF C4, length, Tc/Th, BITS, HUFFVAL
  int n_vals, fell;
};

__device__ __forceinline__ uint64_t ot_freq(const uint32_t* __restrict__ src, int nfreq, int idx) {
  return idx < nfreq ? (uint64_t)src[idx] : (idx == 256 ? 1ull : 0ull);
}

// The table of src[0 .. nfreq) (symbols nfreq..255 do not occur) by the wave of
// w.  Every wave of the workgroup calls this (the barriers are the
// workgroup's); a wave without a table passes nfreq = 0.
__device__ __forceinline__ void ot_build(OtWave& w, const uint32_t* __restrict__ src, int nfreq, int tc_th, int lane) {
  uint64_t f[5];  // entry lane + 64 k (k = 4: the reserved symbol, lane 0)
#pragma unroll
  for (int k = 0; k < 5; ++k) f[k] = (k < 4 || lane == 0) ? ot_freq(src, nfreq, lane + 64 * k) : 0ull;
  for (int i = lane; i < HO_NODES; i += 64) w.parent[i] = 0xFFFF;
  for (int i = lane; i < HO_SYMS; i += 64) w.node[i] = (uint16_t)i;
  if (lane < 33) {
    w.bits[lane] = 0u;
    w.base[lane] = 0u;
  }
  __syncthreads();
  // K.2: merge the two smallest keys until one entry is left (at most 256 steps)
  int next = HO_SYMS;
  for (;;) {
    uint64_t a = HO_DEAD, b = HO_DEAD;
#pragma unroll
    for (int k = 0; k < 5; ++k) ho_min2(a, b, ho_key(f[k], lane + 64 * k), HO_DEAD);
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const uint64_t c = __shfl_xor((unsigned long long)a, o, 64), d = __shfl_xor((unsigned long long)b, o, 64);
      ho_min2(a, b, c, d);
    }
    if (b == HO_DEAD || next >= HO_NODES) break;  // (uniform)
    const int c1 = ho_key_idx(a), c2 = ho_key_idx(b);
    const uint64_t fs = ho_key_freq(a) + ho_key_freq(b);
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      const int idx = lane + 64 * k;
      f[k] = idx == c1 ? fs : (idx == c2 ? 0ull : f[k]);
    }
    if (lane == 0) {  // (this lane alone touches node / parent inside the loop)
      const uint16_t n1 = w.node[c1], n2 = w.node[c2];
      w.parent[n1] = (uint16_t)next;
      w.parent[n2] = (uint16_t)next;
      w.node[c1] = (uint16_t)next;
    }
    ++next;
  }
  __syncthreads();
  // code size = the leaf's depth, every leaf walked by its own lane
  int sz[5], maxd = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) {
    const int idx = lane + 64 * k;
    int d = 0;
    if ((k < 4 || lane == 0) && ot_freq(src, nfreq, idx) != 0ull) {
      int nd = idx;
      while (d < HO_SYMS) {
        const int p = w.parent[nd];
        if (p == 0xFFFF) break;
        nd = p;
        ++d;
      }
    }
    sz[k] = d;
    maxd = d > maxd ? d : maxd;
  }
  const int maxlen = (int)wave_max((uint32_t)maxd);
  const bool fell = maxlen > HO_MAXLEN;  // (uniform)
  if (!fell) {
#pragma unroll
    for (int k = 0; k < 5; ++k) {
      if (sz[k]) {
        atomicAdd(&w.bits[sz[k]], 1u);
        if (k < 4) atomicAdd(&w.base[sz[k]], 1u);
      }
    }
  }
  __syncthreads();
  if (lane == 0) {
    w.fell = fell ? 1 : 0;
    if (!fell) {
      ho_limit(w.bits);
      uint32_t run = 0;
      for (int s = 1; s <= 32; ++s) {
        const uint32_t c = w.base[s];
        w.base[s] = run;
        run += c;
      }
      w.n_vals = (int)run;
      ho_starts(w.bits, w.first, w.cum);
      const int len = 2 + 1 + 16 + (int)run;
      w.dht[0] = 0xFF;
      w.dht[1] = 0xC4;
      w.dht[2] = (uint8_t)(len >> 8);
      w.dht[3] = (uint8_t)(len & 255);
      w.dht[4] = (uint8_t)tc_th;
      for (int l = 1; l <= 16; ++l) w.dht[4 + l] = (uint8_t)w.bits[l];
    } else {
      w.n_vals = 0;
    }
  }
  __syncthreads();
  if (!fell) {
    // HUFFVAL: by size, ascending symbol within a size.  Lane s holds the next
    // position of size s; the symbols go in chunks of 64 in ascending order,
    // the lanes of one size ranked by a ballot.
    uint32_t nextpos = lane < 33 ? w.base[lane] : 0u;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      const int idx = lane + 64 * k, s = sz[k];
      uint32_t pos = 0u;
      unsigned long long rem = __ballot(s > 0);
      while (rem) {  // (uniform)
        const int l0 = __ffsll((long long)rem) - 1;
        const int s0 = __shfl(s, l0, 64);
        const unsigned long long m = __ballot(s == s0);
        const uint32_t b0 = (uint32_t)__shfl((int)nextpos, s0, 64);
        if (s == s0) pos = b0 + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
        if (lane == s0) nextpos += (uint32_t)__popcll(m);
        rem &= ~m;
      }
      if (s > 0) {
        w.dht[ENT_DHT_HEAD + pos] = (uint8_t)idx;
        w.code[idx] = ho_code(pos, w.first, w.cum);
      } else {
        w.code[idx] = 0u;
      }
    }
  }
  __syncthreads();
}

// Frames (sel_freq == nullptr): workgroup f builds frame f's four tables from
// of[f].cnt and writes of[f].es, of[f].hdr, of[f].hdr_len.  A table that falls
// back takes its DHT segment from the frame's header template and its symbols
// from std_tab.  Selftest (sel_freq: n histograms of 256 counts): wave t builds
// table t as an AC table and returns BITS, HUFFVAL, their count and the
// fallback flag.
__global__ void __launch_bounds__(64 * OT_WAVES) k_ent_opt_tables(
    const int n, const uint32_t* __restrict__ sel_freq, uint8_t* __restrict__ sel_bits,
    uint8_t* __restrict__ sel_vals, int32_t* __restrict__ sel_nv, int32_t* __restrict__ sel_fell,
    const EsTab* __restrict__ std_tab, const uint8_t* __restrict__ hdr_std, const long long hdr_stride,
    OptFrame* __restrict__ of) {
  __shared__ OtWave ws[OT_WAVES];
  __shared__ int s_len[OT_WAVES];  // bytes of each table's DHT segment
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  OtWave& w = ws[wv];
  if (sel_freq) {
    const int t = blockIdx.x * OT_WAVES + wv;
    const bool active = t < n;
    ot_build(w, sel_freq + (size_t)(active ? t : 0) * 256, active ? 256 : 0, 0x10, lane);
    if (active) {
      if (lane < 16) sel_bits[(size_t)t * 16 + lane] = w.fell ? 0 : w.dht[5 + lane];
      for (int i = lane; i < 256; i += 64)
        sel_vals[(size_t)t * 256 + i] = (!w.fell && i < w.n_vals) ? w.dht[ENT_DHT_HEAD + i] : 0;
      if (lane == 0) {
        sel_nv[t] = w.n_vals;
        sel_fell[t] = w.fell;
      }
    }
    return;
  }
  const int f = blockIdx.x;
  const int cls = wv >> 1, ac = wv & 1;
  const int tc_th = (ac << 4) | cls;
  OptFrame& o = of[f];
  ot_build(w, o.cnt[cls] + (ac ? 16 : 0), ac ? 256 : 16, tc_th, lane);
  const bool fell = w.fell != 0;
  const int std_nv = ac ? 162 : 12;
  if (lane == 0) s_len[wv] = ENT_DHT_HEAD + (fell ? std_nv : w.n_vals);
  // the frame's symbols
  if (ac) {
    for (int i = lane; i < 16 * ES_RS; i += 64) {
      const int run = i / ES_RS, sz = i % ES_RS;
      o.es.ac[cls][i] = fell ? std_tab->ac[cls][i] : (sz ? es_left(w.code[(run << 4) | sz]) : 0u);
    }
    if (lane == 0) {
      o.es.zrl[cls] = fell ? std_tab->zrl[cls] : es_left(w.code[0xF0]);
      o.es.eob[cls] = fell ? std_tab->eob[cls] : es_left(w.code[0x00]);
    }
  } else if (lane < 16) {
    o.es.dc[cls][lane] = fell ? std_tab->dc[cls][lane] : es_left(w.code[lane]);
  }
  __syncthreads();
  // the header: the template's fixed bytes, then the four DHT segments
  const uint8_t* tmpl = hdr_std + (long long)f * hdr_stride;
  int off = ENT_HDR_FIXED, std_off = ENT_HDR_FIXED;
  for (int t = 0; t < wv; ++t) {
    off += s_len[t];
    std_off += ENT_DHT_HEAD + ((t & 1) ? 162 : 12);
  }
  const int len = s_len[wv];
  for (int i = lane; i < len; i += 64) o.hdr[off + i] = fell ? tmpl[std_off + i] : w.dht[i];
  if (wv == 0) {
    for (int i = lane; i < ENT_HDR_FIXED; i += 64) o.hdr[i] = tmpl[i];
    if (lane == 0) o.hdr_len = (uint32_t)(ENT_HDR_FIXED + s_len[0] + s_len[1] + s_len[2] + s_len[3]);
  }
}

hipError_t launch_opt_tables(int n, const EsTab* std_tab, const uint8_t* hdr_std, long long hdr_stride, OptFrame* of,
                             hipStream_t s) {
  hipLaunchKernelGGL(k_ent_opt_tables, dim3(n), dim3(64 * OT_WAVES), 0, s, n, nullptr, nullptr, nullptr, nullptr,
                     nullptr, std_tab, hdr_std, hdr_stride, of);
  kmark(s, "k_ent_opt_tables");
  return hipGetLastError();
}

// jds_selftest_huffopt_dev: k_ent_opt_tables on n given histograms (device
// pointers; freq: n x 256 counts)
hipError_t launch_opt_tables_selftest(int n, const uint32_t* freq, uint8_t* bits, uint8_t* vals, int32_t* nv,
                                      int32_t* fell, hipStream_t s) {
  const unsigned wg = (unsigned)((n + OT_WAVES - 1) / OT_WAVES);
  hipLaunchKernelGGL(k_ent_opt_tables, dim3(wg), dim3(64 * OT_WAVES), 0, s, n, freq, bits, vals, nv, fell, nullptr,
                     nullptr, 0ll, nullptr);
  return hipGetLastError();
}

// jds_selftest_huffopt: the host builder
void opt_table_host(const uint32_t* freq, HoTable* t) { ho_build_host(freq, t); }

}  // namespace jds
