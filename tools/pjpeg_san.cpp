// pjpeg_san.cpp — the progressive parser (csrc/jds_pjpeg_parse.hpp) and the host
// model of the chain decode (csrc/jds_pjpeg_dec.hpp, the kernel's own core)
// under -fsanitize=address,undefined.  Stand-alone: its own main, no HIP,
// nothing loaded into an interpreter.
//
//   pjpeg_san FILE...          each file once: "<name> rc=<parse rc> status=0x<bits>"
//   pjpeg_san --fuzz FILE...   in addition, per file: every truncation, and every
//                              single-byte substitution from VALUES in its SOS
//                              headers and its scan data
//
// Every input is copied into a heap block of exactly its length and the
// coefficients go to a heap block of exactly coeffs_needed entries between two
// guard words, so a read or write outside either is the sanitizer's report.
// Exit status 0 and a last line "ok": nothing was reported.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "jds_pjpeg_parse.hpp"

using namespace jds;

static const uint8_t VALUES[] = {0x00, 0x01, 0x03, 0x05, 0x11, 0x22, 0x3F, 0xC0,
                                 0xC2, 0xC4, 0xD0, 0xD9, 0xDA, 0xDB, 0xDD, 0xFF};  // tests/golden/make_parse_pins.py

struct Result {
  int rc;
  uint32_t status;
};

static long g_runs = 0, g_parsed = 0, g_defects = 0;

static Result run_one(const uint8_t* bytes, size_t n) {
  uint8_t* d = (uint8_t*)malloc(n ? n : 1);  // exactly n bytes: an over-read is a heap-buffer-overflow
  memcpy(d, bytes, n);
  jds_pjpeg_info* info = (jds_pjpeg_info*)malloc(sizeof(jds_pjpeg_info));
  char msg[512];
  Result r{hd_pjpeg_parse(d, (int64_t)n, info, msg, sizeof msg), 0};
  ++g_runs;
  if (r.rc == JDS_OK && info->frame.H * info->frame.W <= (int64_t)1 << 28) {
    ++g_parsed;
    const size_t nc = (size_t)info->frame.coeffs_needed;
    int16_t* cf = (int16_t*)malloc(sizeof(int16_t) * (nc + 2));
    cf[0] = cf[nc + 1] = 0x5A5A;
    r.status = hd_pjpeg_host_decode(d, (int64_t)n, info, cf + 1);
    if (cf[0] != 0x5A5A || cf[nc + 1] != 0x5A5A) {
      fprintf(stderr, "guard word overwritten\n");
      abort();
    }
    if (r.status) ++g_defects;
    free(cf);
  }
  free(info);
  free(d);
  return r;
}

static bool read_file(const char* path, std::vector<uint8_t>& out) {
  FILE* f = fopen(path, "rb");
  if (!f) return false;
  uint8_t buf[65536];
  size_t n;
  while ((n = fread(buf, 1, sizeof buf, f)) > 0) out.insert(out.end(), buf, buf + n);
  fclose(f);
  return true;
}

int main(int argc, char** argv) {
  bool fuzz = false;
  for (int a = 1; a < argc; ++a) {
    if (!strcmp(argv[a], "--fuzz")) {
      fuzz = true;
      continue;
    }
    std::vector<uint8_t> file;
    if (!read_file(argv[a], file)) {
      fprintf(stderr, "cannot read %s\n", argv[a]);
      return 2;
    }
    const Result r = run_one(file.data(), file.size());
    printf("%s rc=%d status=0x%x\n", argv[a], r.rc, r.status);
    if (!fuzz) continue;
    for (size_t n = 0; n < file.size(); ++n) run_one(file.data(), n);
    jds_pjpeg_info* info = (jds_pjpeg_info*)malloc(sizeof(jds_pjpeg_info));
    char msg[512];
    if (hd_pjpeg_parse(file.data(), (int64_t)file.size(), info, msg, sizeof msg) == JDS_OK) {
      std::vector<uint8_t> m = file;
      for (int s = 0; s < info->n_scans; ++s) {
        // the SOS segment (marker, length, 1 + 2 Ns + 3 bytes) and the entropy-coded bytes behind it
        const int64_t a0 = info->scan[s].offset - (6 + 2 * info->scan[s].n_components);
        const int64_t a1 = info->scan[s].offset + info->scan[s].length;
        for (int64_t p = a0 < 0 ? 0 : a0; p < a1; ++p)
          for (uint8_t v : VALUES) {
            if (m[(size_t)p] == v) continue;
            const uint8_t keep = m[(size_t)p];
            m[(size_t)p] = v;
            run_one(m.data(), m.size());
            m[(size_t)p] = keep;
          }
      }
    }
    free(info);
  }
  printf("runs=%ld parsed=%ld defects=%ld\nok\n", g_runs, g_parsed, g_defects);
  return 0;
}
