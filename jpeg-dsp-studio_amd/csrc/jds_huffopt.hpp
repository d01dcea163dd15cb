// jds_huffopt.hpp — the core of the optimised Huffman tables (DESIGN.md
// "Optimised tables"; byte-for-byte definition: tests/huffopt_ref.py).
// Compiles for host and device: k_ent_opt_tables (jds_huffopt.hip, one wave per
// table), the host builder behind jds_selftest_huffopt and the stand-alone
// sanitizer program (tools/huffopt_host_san.cpp) share the merge order (ho_key),
// the length limiter (ho_limit) and the code assignment (ho_starts, ho_code).
// No HIP types here.
//
// The construction is T.81 K.2 with libjpeg's tie rules.  freq[256] = 1 is the
// reserved symbol (no code is all ones).  Each step merges the two live entries
// of least frequency, the LARGEST index winning a tie, the second into the
// first's index.  K.2 keeps the merged symbols on `others` chains and adds one
// bit along both chains per merge; a symbol's final code size is therefore its
// leaf's depth in the merge tree, so the builders here record parent pointers
// (node 257 + step is the parent of the two entries' current nodes) and walk
// every leaf up to the root afterwards -- in parallel on the device.
#pragma once
#include <stdint.h>

#ifdef __HIPCC__
#define JDS_HO __host__ __device__ __forceinline__
#else
#define JDS_HO inline
#endif

namespace jds {

constexpr int HO_SYMS = 257;             // 256 symbols + the reserved one
constexpr int HO_NODES = 2 * HO_SYMS;    // leaves + at most 256 merges
constexpr int HO_MAXLEN = 32;            // longer than this before limiting: the class falls back to Annex K
constexpr uint64_t HO_DEAD = ~0ull;

// Order of the merge: the smaller key is the smaller frequency, and among equal
// frequencies the LARGER index (K.2 scans 0..256 with <=).  freq < 2^55.
JDS_HO uint64_t ho_key(uint64_t freq, int idx) { return freq ? (freq << 9) | (uint64_t)(511 - idx) : HO_DEAD; }
JDS_HO int ho_key_idx(uint64_t key) { return 511 - (int)(key & 511u); }
JDS_HO uint64_t ho_key_freq(uint64_t key) { return key >> 9; }

// (a, b) <- the two smallest of {a, b, c, d} where a < b and c < d (or dead)
JDS_HO void ho_min2(uint64_t& a, uint64_t& b, uint64_t c, uint64_t d) {
  const uint64_t lo = a < c ? a : c, hi = a < c ? c : a;
  const uint64_t m = b < d ? b : d;
  a = lo;
  b = hi < m ? hi : m;
}

// T.81 K.3 (Adjust_BITS) on bits[0..32]: no code longer than 16 bits, then the
// reserved symbol's code -- the longest -- taken off.
JDS_HO void ho_limit(uint32_t* bits) {
  for (int i = 32; i > 16; --i) {
    while (bits[i] > 0) {
      int j = i - 2;
      while (bits[j] == 0) --j;
      bits[i] -= 2;
      bits[i - 1] += 1;
      bits[j + 1] += 2;
      bits[j] -= 1;
    }
  }
  int i = 16;
  while (i > 0 && bits[i] == 0) --i;
  if (i > 0) bits[i] -= 1;
}

// T.81 Annex C: first[l] = the first code of length l, cum[l] = the HUFFVAL
// position of that code (cum[17] = the number of values)
JDS_HO void ho_starts(const uint32_t* bits, uint32_t* first, uint32_t* cum) {
  uint32_t code = 0, k = 0;
  first[0] = 0;
  cum[0] = 0;
  for (int l = 1; l <= 16; ++l) {
    first[l] = code;
    cum[l] = k;
    code = (code + bits[l]) << 1;
    k += bits[l];
  }
  cum[17] = k;
}

// the code of HUFFVAL position pos as length << 16 | code
JDS_HO uint32_t ho_code(uint32_t pos, const uint32_t* first, const uint32_t* cum) {
  int l = 1;
  while (l < 16 && pos >= cum[l + 1]) ++l;
  return ((uint32_t)l << 16) | (first[l] + (pos - cum[l]));
}

struct HoTable {
  uint8_t bits[16];     // BITS[1..16]
  uint8_t vals[256];    // HUFFVAL
  int32_t n_vals;
  int32_t fell_back;    // a code would exceed HO_MAXLEN bits: nothing else is set
  int32_t max_len;      // the longest code before limiting (the reserved symbol included)
  uint32_t code[256];   // symbol -> length << 16 | code (0: not in the table)
};

// The whole construction on the host, with the device's data structures.
inline void ho_build_host(const uint32_t* freq, HoTable* t) {
  uint64_t f[HO_SYMS];
  uint16_t node[HO_SYMS], parent[HO_NODES];
  for (int i = 0; i < 256; ++i) f[i] = freq[i];
  f[256] = 1;
  for (int i = 0; i < HO_SYMS; ++i) node[i] = (uint16_t)i;
  for (int i = 0; i < HO_NODES; ++i) parent[i] = 0xFFFF;
  int next = HO_SYMS;
  for (;;) {
    uint64_t a = HO_DEAD, b = HO_DEAD;
    for (int i = 0; i < HO_SYMS; ++i) ho_min2(a, b, ho_key(f[i], i), HO_DEAD);
    if (b == HO_DEAD) break;
    const int c1 = ho_key_idx(a), c2 = ho_key_idx(b);
    f[c1] = ho_key_freq(a) + ho_key_freq(b);
    f[c2] = 0;
    parent[node[c1]] = parent[node[c2]] = (uint16_t)next;
    node[c1] = (uint16_t)next++;
  }
  uint8_t size[HO_SYMS];
  int maxlen = 0;
  for (int i = 0; i < HO_SYMS; ++i) {
    int d = 0;
    if (i == 256 || freq[i])
      for (int n = i; parent[n] != 0xFFFF; n = parent[n]) ++d;
    size[i] = (uint8_t)d;
    maxlen = d > maxlen ? d : maxlen;
  }
  *t = HoTable{};
  t->max_len = maxlen;
  if (maxlen > HO_MAXLEN) {
    t->fell_back = 1;
    return;
  }
  uint32_t bits[33] = {0}, first[18], cum[18];
  for (int i = 0; i < HO_SYMS; ++i)
    if (size[i]) bits[size[i]]++;
  ho_limit(bits);
  ho_starts(bits, first, cum);
  int k = 0;
  for (int s = 1; s <= 32; ++s)
    for (int i = 0; i < 256; ++i)
      if (size[i] == s) {
        t->code[i] = ho_code((uint32_t)k, first, cum);
        t->vals[k++] = (uint8_t)i;
      }
  t->n_vals = k;
  for (int l = 1; l <= 16; ++l) t->bits[l - 1] = (uint8_t)bits[l];
}

}  // namespace jds
