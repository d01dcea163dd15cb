// jds_entropy_mcu_dev.hpp — the interleaved-scan writer's launch interface
// (jds_entropy_mcu.hip) as the C-ABI sees it: the device arrays of one batch
// and the two groups of launches around the host's read of the files' lengths.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "jds_entropy_common.hpp"
#include "jds_entropy_mcu.hpp"

namespace jds {

// files, segfile and pfx are uploaded by the caller; the rest is scratch
// carved from one allocation (mcu_carve).
struct McuDev {
  const McuFile* files;      // per file
  const int32_t* segfile;    // per segment: its file
  const uint8_t* pfx;        // the files' header prefixes (McuFile::pfx_off)
  // per segment (k_ent_walk's arrays): end bit within the file's scan, bit
  // total, file-relative prefix of the totals (long scans), 0xFF bytes and
  // their prefix, first output byte within the file, per-lane bits, error flag
  unsigned long long *desc, *agg, *segoff, *ffs, *ffx, *outoff;
  uint32_t *nbits, *badseg;
  // per file: scan bits, file length, "not baseline-codable", first byte in the output (< 0: not written)
  unsigned long long *fbits, *flen;
  uint32_t* fbad;
  long long* fout;
  OptFrame* of;      // the files' code tables (nf + 1 frames)
  uint8_t* hdr_std;  // a header template: what a table class falls back to (ENT_HDR bytes)
  uint32_t* raw;     // the packed scans
  uint32_t* gst;     // the staged words, word-major per segment
};

long long mcu_raw_words(int nblk);
long long mcu_capacity(const McuFile& f);
size_t mcu_carve(void* base, int nf, long long nseg, long long raw_words, McuDev* d);
size_t mcu_scratch_bytes(int nf, long long nseg, long long raw_words);
size_t mcu_optframe_bytes();
void mcu_std_frame(const EsTab* es_host, const uint8_t* hdr_std, void* out);
int mcu_self_max();
hipError_t launch_mcu_code(const McuDev& d, int nf, int nseg, bool any_long, const int16_t* coeffs, bool optimize,
                           const EsTab* std_tab, hipStream_t s);
hipError_t launch_mcu_emit(const McuDev& d, int nf, int nseg, uint8_t* out, hipStream_t s);

// jds_entropy.hip: the left-aligned symbols behind the Annex K table object
const EsTab* ent_es_tab(const void* tab);

}  // namespace jds
