// jpeg_splice_san.cpp — stand-alone host program over the transcode's header
// splicer (csrc/jds_entropy_mcu.hpp: mcu_splice) and the parser beside it
// (csrc/jds_jpeg_parse.hpp: hd_jpeg_parse), for sanitizer runs:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all \
//       -Iinclude -Ijpeg-dsp-studio_amd/csrc tools/jpeg_splice_san.cpp -o jpeg_splice_san
//   ./jpeg_splice_san [seed]
//
// Writes small files of every subsampling mode with the writer's host model
// (mcu_host_write: the kernels' block lookup and predecessor rule over an
// exactly-sized coefficient array, so an index outside a plane is a sanitizer
// report), APPn and COM segments in their prefixes, and drives the parser and
// the splicer -- every input in a heap block of exactly its length, every
// output in one of exactly the reported size -- over
//   * the file itself: it parses, the spliced prefix is the one written;
//   * the file truncated at every byte;
//   * every segment's length field set to 0, 1, one past the end, 0xFFFF;
//   * hostile DHT segments: BITS that over-subscribe the code space, that sum
//     past 256 symbols, that sum past the segment, table classes and ids out
//     of range, a DHT that ends inside its BITS;
//   * random byte changes in the header region.
// Checked besides the sanitizers: whatever the parser accepts, the splicer
// accepts; a prefix holds no DHT and no DRI segment and never more bytes than
// the file's header; an output buffer one byte short is refused.
// No HIP, no GPU.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "jds_entropy_mcu.hpp"
#include "jds_jpeg_parse.hpp"

static uint64_t g_rng = 0x9e3779b97f4a7c15ull;
static uint32_t rnd() {
  g_rng ^= g_rng << 13;
  g_rng ^= g_rng >> 7;
  g_rng ^= g_rng << 17;
  return (uint32_t)(g_rng >> 16);
}

static long g_runs = 0, g_parsed = 0, g_spliced = 0;

// the prefix holds whole segments, none of them DHT or DRI
static bool prefix_clean(const uint8_t* p, int64_t n) {
  int64_t i = 0;
  while (i < n) {
    if (i + 4 > n || p[i] != 0xFF || p[i + 1] == 0xC4 || p[i + 1] == 0xDD) return false;
    i += 2 + (((int64_t)p[i + 2] << 8) | p[i + 3]);
  }
  return i == n;
}

// parser and splicer on a heap copy of exactly `len` bytes; 0 ok
static int drive(const uint8_t* src, int64_t len, std::vector<uint8_t>* pfx_out) {
  uint8_t* d = (uint8_t*)malloc(len > 0 ? (size_t)len : 1);
  if (!d) return 1;
  if (len > 0) memcpy(d, src, (size_t)len);
  ++g_runs;
  jds_jpeg_info info;
  char msg[256];
  const int rc = jds::hd_jpeg_parse(d, len, &info, msg, sizeof msg);
  const int64_t n = jds::mcu_splice(d, len, nullptr, 0);
  int bad = 0;
  if (rc == JDS_OK) ++g_parsed;
  if (rc == JDS_OK && n < 0) bad = 1;  // the parser accepted what the splicer does not
  if (n >= 0) {
    ++g_spliced;
    if (n > len) bad = 2;
    uint8_t* o = (uint8_t*)malloc(n > 0 ? (size_t)n : 1);
    if (!o) return 1;
    if (jds::mcu_splice(d, len, o, n) != n) bad = 3;
    if (!bad && !prefix_clean(o, n)) bad = 4;
    if (n > 0 && jds::mcu_splice(d, len, o, n - 1) != -1) bad = 5;  // one byte short
    if (pfx_out) pfx_out->assign(o, o + n);
    free(o);
  }
  if (rc == JDS_OK && !bad && info.H * info.W <= (int64_t)1 << 28) {  // (jds_jpeg_parse's size limit)
    jds::McuFile f;
    if (jds::mcu_file_of(&info, &f) != 0) bad = 6;  // the parser's grids are T.81's
  }
  free(d);
  if (bad) fprintf(stderr, "check %d failed on a file of %lld bytes\n", bad, (long long)len);
  return bad;
}

static void put_seg(std::vector<uint8_t>& v, int marker, const std::vector<uint8_t>& body) {
  const int ln = 2 + (int)body.size();
  v.push_back(0xFF);
  v.push_back((uint8_t)marker);
  v.push_back((uint8_t)(ln >> 8));
  v.push_back((uint8_t)(ln & 255));
  v.insert(v.end(), body.begin(), body.end());
}

// placeholder standard tables (what a table class would fall back to; the small scans here never do)
static uint8_t g_dc_bits[16], g_ac_bits[16], g_dc_vals[12], g_ac_vals[162];

static int make_file(int H, int W, int ss, std::vector<uint8_t>* file, std::vector<uint8_t>* prefix) {
  jds_jpeg_info info;
  memset(&info, 0, sizeof info);
  info.H = H;
  info.W = W;
  info.subsampling = ss;
  const int vmax = ss == JDS_SS_420 ? 2 : 1, hmax = ss == JDS_SS_444 ? 1 : 2;
  for (int c = 0; c < 3; ++c) {
    const int h = c ? (H + vmax - 1) / vmax : H, w = c ? (W + hmax - 1) / hmax : W;
    info.grid_rows[c] = (h + 7) / 8;
    info.grid_cols[c] = (w + 7) / 8;
    info.coeffs_needed += 64 * info.grid_rows[c] * info.grid_cols[c];
    info.tq[c] = c ? 1 : 0;
    for (int i = 0; i < 64; ++i) info.qtable[c][i] = 1 + rnd() % 255;
  }
  jds::McuFile f;
  if (jds::mcu_file_of(&info, &f) != 0 || jds::mcu_coeffs(f) != info.coeffs_needed) return 1;
  int16_t* cf = (int16_t*)malloc(sizeof(int16_t) * (size_t)info.coeffs_needed);
  if (!cf) return 1;
  for (int64_t i = 0; i < info.coeffs_needed; ++i)
    cf[i] = (i % 64 == 0 || rnd() % 10 < 3) ? (int16_t)((int)(rnd() % 401) - 200) : (int16_t)0;
  uint8_t head[jds::MCU_PFX_DEFAULT_MAX];
  const int hn = jds::mcu_default_prefix(&info, head);
  if (hn < 0) return 1;
  prefix->clear();
  std::vector<uint8_t> exif(40 + rnd() % 300), com(rnd() % 40);
  for (uint8_t& b : exif) b = (uint8_t)rnd();  // (0xFF bytes included: a segment's body is opaque)
  for (uint8_t& b : com) b = (uint8_t)rnd();
  prefix->insert(prefix->end(), head, head + 18);  // APP0
  put_seg(*prefix, 0xE1, exif);
  put_seg(*prefix, 0xFE, com);
  prefix->insert(prefix->end(), head + 18, head + hn);  // DQT.., SOF0
  jds::McuStdTabs st;
  for (int t = 0; t < 4; ++t) {
    st.bits[t] = (t & 1) ? g_ac_bits : g_dc_bits;
    st.vals[t] = (t & 1) ? g_ac_vals : g_dc_vals;
    st.n_vals[t] = (t & 1) ? 162 : 12;
  }
  const int rc = jds::mcu_host_write(f, cf, 1, prefix->data(), (int64_t)prefix->size(), st, file);
  free(cf);
  return rc;
}

static int over(const std::vector<uint8_t>& file) {
  int bad = 0;
  const int64_t len = (int64_t)file.size();
  // truncated at every byte
  for (int64_t l = 0; l <= len && !bad; ++l) bad = drive(file.data(), l, nullptr);
  // the segments of the header
  std::vector<int64_t> segs;
  for (int64_t p = 2; p + 4 <= len && file[(size_t)p] == 0xFF && file[(size_t)p + 1] != 0xDA;
       p += 2 + (((int64_t)file[(size_t)p + 2] << 8) | file[(size_t)p + 3]))
    segs.push_back(p);
  int64_t sos = segs.empty() ? 2 : segs.back() + 2 + (((int64_t)file[(size_t)segs.back() + 2] << 8) | file[(size_t)segs.back() + 3]);
  for (int64_t p : segs) {
    const int64_t past = len - p - 2 + 1;
    for (int64_t v : {(int64_t)0, (int64_t)1, past, (int64_t)0xFFFF, past - 1}) {
      if (v < 0 || v > 0xFFFF) continue;
      std::vector<uint8_t> m(file);
      m[(size_t)p + 2] = (uint8_t)(v >> 8);
      m[(size_t)p + 3] = (uint8_t)(v & 255);
      if (!bad) bad = drive(m.data(), len, nullptr);
    }
    if (file[(size_t)p + 1] != 0xC4) continue;
    // hostile tables
    const size_t b0 = (size_t)p + 5;  // BITS
    for (int kind = 0; kind < 6 && !bad; ++kind) {
      std::vector<uint8_t> m(file);
      switch (kind) {
        case 0: m[b0] = 3; break;                                     // three codes of one bit
        case 1: for (int i = 0; i < 16; ++i) m[b0 + i] = 17; break;   // 272 symbols
        case 2: m[b0 + 15] = 255; break;                              // past the segment
        case 3: m[b0 - 1] = 0x20; break;                              // table class 2
        case 4: m[b0 - 1] = 0x04; break;                              // table id 4
        default: m[(size_t)p + 2] = 0; m[(size_t)p + 3] = 10; break;  // ends inside BITS
      }
      bad = drive(m.data(), len, nullptr);
    }
  }
  // random changes in the header region
  for (int it = 0; it < 400 && !bad; ++it) {
    std::vector<uint8_t> m(file);
    const int nchg = 1 + (int)(rnd() % 3);
    for (int j = 0; j < nchg; ++j) m[(size_t)(rnd() % (uint32_t)sos)] = (rnd() & 1) ? 0xFF : (uint8_t)rnd();
    bad = drive(m.data(), len, nullptr);
  }
  return bad;
}

int main(int argc, char** argv) {
  if (argc > 1) g_rng ^= (uint64_t)atoll(argv[1]) * 0x2545f4914f6cdd1dull;
  g_dc_bits[3] = 12;
  g_ac_bits[7] = 162;
  for (int i = 0; i < 12; ++i) g_dc_vals[i] = (uint8_t)i;
  for (int i = 0; i < 162; ++i) g_ac_vals[i] = (uint8_t)i;
  const int sizes[][2] = {{1, 1}, {8, 8}, {17, 33}, {37, 53}, {16, 40}};
  long failed = 0, files = 0;
  for (int ss = 0; ss < 3; ++ss)
    for (const auto& s : sizes) {
      std::vector<uint8_t> file, prefix, got;
      if (make_file(s[0], s[1], ss, &file, &prefix)) {
        fprintf(stderr, "%dx%d mode %d: the host model did not write a file\n", s[0], s[1], ss);
        ++failed;
        continue;
      }
      ++files;
      const long parsed0 = g_parsed;
      int bad = drive(file.data(), (int64_t)file.size(), &got);
      if (!bad && (g_parsed == parsed0 || got != prefix)) {
        fprintf(stderr, "%dx%d mode %d: the written file does not parse or its prefix differs\n", s[0], s[1], ss);
        bad = 1;
      }
      if (!bad) bad = over(file);
      failed += bad != 0;
    }
  printf("%ld files, %ld inputs through the parser and the splicer (%ld parsed, %ld spliced), %ld failed: %s\n", files,
         g_runs, g_parsed, g_spliced, failed, failed ? "FAILED" : "ok");
  return failed ? 1 : 0;
}
