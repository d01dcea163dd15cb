// hd_window_check.cpp — stand-alone host check of the decode core's destuffing
// window and of the positions hd_run visits (csrc/jds_huffdec.hpp), for
// sanitizer runs:
//
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ijpeg-dsp-studio_amd/csrc tools/hd_window_check.cpp -o hd_window_check
//   ./hd_window_check
//
// 1. hd_window(HdMemSrc{d, n}, b, w, ffm) against a byte-by-byte walk that takes
//    five data bytes from b (a stuffed byte after every in-range 0xFF skipped
//    and recorded in ffm, bytes at or past n read as 0xFF data), for every
//    data-byte position b of seeded buffers: 1..40 data bytes, 0xFF among them
//    with probability 0, 0.1, 0.5, 0.9 and 1, every 0xFF followed by its 0x00,
//    and buffers that end right after an 0xFF, its stuffing cut off.
// 2. hd_run, one symbol per call, over scans written here with two ladder
//    tables: nine symbols, the last code 11111111, every AC coefficient 255 and
//    the DC alternating 255 / 0; and seventeen symbols, 1023 on the 16-bit
//    all-ones code and DC differences of +-2047 (symbols of 26 and 27 bits, five
//    data bytes each).  All but a few data bytes of these scans are 0xFF.  Then
//    random symbols of the same tables.  After every symbol the position must
//    be the naive one (the destuffed bit count mapped through the stuffed byte
//    offsets) and the sink must have seen the written coefficient.
//
// Every buffer is an exactly sized heap copy, so a read past its end is a
// sanitizer report.  Exits non-zero at the first mismatch and prints the case.
// No HIP, no GPU.
#include <stdio.h>
#include <stdlib.h>

#include <vector>

#include "jds_huffdec.hpp"

namespace {

struct Rng {  // xorshift64*
  uint64_t s;
  uint32_t next() {
    s ^= s >> 12;
    s ^= s << 25;
    s ^= s >> 27;
    return (uint32_t)((s * 0x2545F4914F6CDD1Dull) >> 32);
  }
  double unit() { return next() / 4294967296.0; }
};

void print_bytes(const uint8_t* d, int64_t n) {
  for (int64_t i = 0; i < n; ++i) fprintf(stderr, "%02X ", d[i]);
  fprintf(stderr, "\n");
}

void naive_window(const uint8_t* d, int64_t n, int64_t b, uint64_t& w, uint32_t& ffm) {
  w = 0;
  ffm = 0;
  int64_t j = b;
  for (int cnt = 0; cnt < 5; ++cnt) {
    uint32_t v = 0xFF;
    if (j < n) {
      v = d[j];
      if (v == 0xFF) {
        ffm |= 1u << cnt;
        ++j;  // its stuffed byte (perhaps cut off)
      }
    }
    ++j;
    w = (w << 8) | v;
  }
}

// every data-byte position of one stuffed buffer, from an exactly sized heap copy
long check_buffer(const std::vector<uint8_t>& buf, const std::vector<int64_t>& data_pos, const char* what) {
  const int64_t n = (int64_t)buf.size();
  uint8_t* d = (uint8_t*)malloc((size_t)n);
  if (!d) exit(2);
  memcpy(d, buf.data(), (size_t)n);
  long checked = 0;
  for (int64_t b : data_pos) {
    uint64_t w, w0;
    uint32_t ffm, ffm0;
    jds::hd_window(jds::HdMemSrc{d, n}, b, w, ffm);
    naive_window(d, n, b, w0, ffm0);
    if (w != w0 || ffm != ffm0) {
      fprintf(stderr, "hd_window mismatch (%s): n %lld, b %lld: w %010llX ffm %02X, expected w %010llX ffm %02X\nbuffer: ",
              what, (long long)n, (long long)b, (unsigned long long)w, ffm, (unsigned long long)w0, ffm0);
      print_bytes(d, n);
      exit(1);
    }
    ++checked;
  }
  free(d);
  return checked;
}

long check_windows() {
  const double probs[5] = {0.0, 0.1, 0.5, 0.9, 1.0};
  Rng rng{0x9E3779B97F4A7C15ull};
  long checked = 0;
  for (int len = 1; len <= 40; ++len)
    for (double p : probs)
      for (int rep = 0; rep < 24; ++rep) {
        std::vector<uint8_t> buf;
        std::vector<int64_t> pos;
        for (int i = 0; i < len; ++i) {
          uint8_t v = rng.unit() < p ? 0xFF : (uint8_t)(rng.next() % 255u);  // 0x00 .. 0xFE
          if (rep % 3 == 2 && i == len - 1) v = 0xFF;                        // ends in an 0xFF
          pos.push_back((int64_t)buf.size());
          buf.push_back(v);
          if (v == 0xFF) buf.push_back(0x00);
        }
        checked += check_buffer(buf, pos, "stuffed");
        if (buf.size() >= 2 && buf[buf.size() - 2] == 0xFF) {
          buf.pop_back();  // the last 0xFF's stuffing cut off
          checked += check_buffer(buf, pos, "cut after 0xFF");
        }
      }
  return checked;
}

// MSB-first bit writer with stuffing; data_at[i]: the stuffed offset of data byte i
struct Bits {
  std::vector<uint8_t> out;
  std::vector<int64_t> data_at;
  uint32_t acc = 0;
  int n = 0;
  uint64_t total = 0;
  void put(uint32_t v, int len) {
    for (int i = len - 1; i >= 0; --i) {
      acc = (acc << 1) | ((v >> i) & 1u);
      ++total;
      if (++n == 8) {
        data_at.push_back((int64_t)out.size());
        out.push_back((uint8_t)acc);
        if ((uint8_t)acc == 0xFF) out.push_back(0x00);
        acc = 0;
        n = 0;
      }
    }
  }
  void flush() {
    const uint64_t t = total;
    while (n) put(1, 1);
    total = t;
    data_at.push_back((int64_t)out.size());
  }
  uint64_t stuffed_pos(uint64_t bit) const { return 8u * (uint64_t)data_at[bit >> 3] + (bit & 7u); }
};

struct Sym {
  int blk, k, val;
  uint64_t end;  // destuffed bits up to and including this symbol
};

struct CheckSink {
  int blk = -1, k = -1, val = 0, calls = 0;
  void operator()(int64_t b, int kk, int v) {
    blk = (int)b;
    k = kk;
    val = v;
    ++calls;
  }
};

// A ladder code: one code of every length 1 .. L - 1 (i ones and a zero) and two of
// length L, the last of them all ones.  dc0: the index of DC category 0 (the
// categories follow in order); pm1: the index of AC symbol 0x01.
struct Ladder {
  int L;
  uint8_t bits[16];
  uint8_t dc[17], ac[17];
  int dc0, pm1;
  int top;          // the value whose magnitude bits are all ones, on the all-ones AC code
  int dc_a, dc_b;   // the dense scan's alternating DC values
  int n() const { return L + 1; }
};

const Ladder L8 = {8, {1, 1, 1, 1, 1, 1, 1, 2, 0, 0, 0, 0, 0, 0, 0, 0},
                   {0, 1, 2, 3, 4, 5, 6, 7, 8},
                   {0x00, 0x01, 0x11, 0x02, 0x03, 0x04, 0xF0, 0x07, 0x08}, 0, 1, 255, 255, 0};
// 1023 on the 16-bit all-ones code: 26 one-bits a coefficient, 27 for a DC difference of 2047
const Ladder L16 = {16, {1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 2},
                    {12, 13, 14, 15, 16, 0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11},
                    {0x01, 0x11, 0x21, 0x02, 0x03, 0x04, 0x05, 0x06, 0x07, 0x08, 0x09, 0xF0, 0x31, 0x41, 0x00, 0x1A, 0x0A},
                    5, 0, 1023, 1023, -1024};

void put_code(Bits& w, const Ladder& t, int i) {
  if (i == t.L)
    w.put((1u << t.L) - 1u, t.L);
  else
    w.put((1u << (i + 1)) - 2u, i + 1);
}

void put_value(Bits& w, int v, int size) { w.put((uint32_t)(v < 0 ? v - 1 : v) & ((1u << size) - 1u), size); }

int size_of(int v) {
  int a = v < 0 ? -v : v, s = 0;
  while (a) {
    ++s;
    a >>= 1;
  }
  return s;
}

long check_run(const Ladder& t, bool dense, int nblocks, uint64_t seed) {
  Rng rng{seed};
  Bits w;
  std::vector<Sym> syms;
  int pred = 0;
  const int half = t.L == 8 ? 127 : 1000;  // any two DC values differ by a category the table holds
  for (int b = 0; b < nblocks; ++b) {
    const int dc = dense ? ((b & 1) ? t.dc_b : t.dc_a) : (int)(rng.next() % (uint32_t)(2 * half + 1)) - half;
    const int diff = dc - pred, ds = size_of(diff);
    pred = dc;
    put_code(w, t, t.dc0 + ds);
    put_value(w, diff, ds);
    syms.push_back({b, 0, diff, w.total});
    int k = 1;
    while (k < 64) {
      int i = dense ? t.L : (int)(rng.next() % (uint32_t)t.n());
      if (!dense && rng.unit() < 0.5) i = t.L;
      const int sym = t.ac[i], run = sym >> 4, size = sym & 15;
      if (sym == 0xF0) {
        if (k + 16 > 62) continue;  // a ZRL must leave room for the coefficient it leads to
        put_code(w, t, i);
        k += 16;
        syms.push_back({b, -1, 0, w.total});
        put_code(w, t, t.pm1);  // then a +-1
        const int v = (rng.next() & 1u) ? 1 : -1;
        put_value(w, v, 1);
        syms.push_back({b, k, v, w.total});
        ++k;
        continue;
      }
      if (sym == 0x00) {
        put_code(w, t, i);
        syms.push_back({b, -1, 0, w.total});
        break;
      }
      if (k + run > 63) continue;
      int v = dense ? t.top : (int)((1u << (size - 1)) + rng.next() % (1u << (size - 1)));
      if (!dense && (rng.next() & 1u)) v = -v;
      if (!dense && i == t.L && rng.unit() < 0.7) v = t.top;
      put_code(w, t, i);
      put_value(w, v, size);
      k += run;
      syms.push_back({b, k, v, w.total});
      ++k;
    }
  }
  w.flush();
  const int64_t n = (int64_t)w.out.size();
  uint8_t* d = (uint8_t*)malloc((size_t)n);
  if (!d) exit(2);
  memcpy(d, w.out.data(), (size_t)n);
  if (dense) {
    long ff = 0;
    for (int64_t i = 0; i < n; ++i) ff += d[i] == 0xFF;
    if (2 * ff < n - n / 8) {
      fprintf(stderr, "the dense scan is not dense: %ld of %lld bytes are 0xFF\n", ff, (long long)n);
      exit(1);
    }
  }
  jds::HuffDecTab dct, act;
  if (jds::hd_build(t.bits, t.dc, &dct) != t.n() || jds::hd_build(t.bits, t.ac, &act) != t.n()) {
    fprintf(stderr, "hd_build rejects the ladder table\n");
    exit(1);
  }
  const jds::HdMemSrc src{d, n};
  const jds::HdPlain tc{&dct, &act};
  uint64_t p = 0;
  int k = 0, slot = 0;
  int64_t blk = 0;
  for (size_t i = 0; i < syms.size(); ++i) {
    CheckSink sink;
    const uint64_t p0 = p;
    const uint32_t fl = jds::hd_run(src, tc, p, k, slot, p + 1, blk, (int64_t)nblocks, sink);  // one symbol
    const uint64_t want = w.stuffed_pos(syms[i].end);
    const bool coef = syms[i].k >= 0;
    if (fl || p != want || sink.calls != (coef ? 1 : 0) ||
        (coef && (sink.blk != syms[i].blk || sink.k != syms[i].k || sink.val != syms[i].val))) {
      fprintf(stderr,
              "hd_run mismatch (%d-bit ladder, %s scan, seed %llu): symbol %zu from bit %llu: status 0x%x, position %llu (expected %llu), "
              "sink (%d, %d, %d) x%d, expected (%d, %d, %d)\nbytes from there: ",
              t.L, dense ? "dense" : "mixed", (unsigned long long)seed, i, (unsigned long long)p0, fl, (unsigned long long)p,
              (unsigned long long)want, sink.blk, sink.k, sink.val, sink.calls, syms[i].blk, syms[i].k, syms[i].val);
      print_bytes(d + (p0 >> 3), n - (int64_t)(p0 >> 3) < 12 ? n - (int64_t)(p0 >> 3) : 12);
      exit(1);
    }
  }
  if (blk != nblocks || k != 0 || !jds::hd_tail_ok(src, p)) {
    fprintf(stderr, "hd_run (%s scan): %lld of %d blocks, k %d, tail at bit %llu of %lld bytes\n", dense ? "dense" : "mixed",
            (long long)blk, nblocks, k, (unsigned long long)p, (long long)n);
    exit(1);
  }
  free(d);
  return (long)syms.size();
}

}  // namespace

int main() {
  const long windows = check_windows();
  long symbols = 0;
  for (const Ladder* t : {&L8, &L16}) {
    symbols += check_run(*t, true, 24, 1);
    for (uint64_t seed = 2; seed < 12; ++seed) symbols += check_run(*t, false, 40, seed);
  }
  printf("%ld windows, %ld symbols: all as the naive walk\n", windows, symbols);
  return 0;
}
