// jds_dec_jobs.hpp — from a parsed file to the decode kernels' work lists.
//
// Host only and HIP-free (plain C++, like jds_jpeg_parse.hpp):
// the index arithmetic that decides which bytes every decode workgroup reads
// and where its blocks go.  The batch driver in jds_abi_jpeg.hip calls it (a
// single file is its batch of one); tools/dec_jobs_san.cpp runs it under the host sanitizers.
#pragma once

#include <stdint.h>
#include <string.h>

#include <vector>

#include "jds_jpeg_parse.hpp"

namespace jds {

// Where a file's descriptors point in launches that serve several files
// (jds_jpeg_batch_to_rgb); a single-file call is the batch of one, placed at zeros.
struct FilePlace {
  int file;            // its table set (tabs + 4 * file), MCU record (mcu + file) and status word
  long long data_off;  // its first byte, from the files base
  long long coef_off;  // its first coefficient, from the coeffs base
  long long dcs_off;   // interleaved: its first entry in the DC staging array
};

// What the builder reads of a parsed file.  A non-interleaved scan holds its
// component's T.81 grid (A.2.2): coef_off is the component's plane within the
// file, tables by id.  The one interleaved scan holds whole MCUs of all
// components: its blocks find their planes and tables through the file's HdMcu.
struct DecJobScan {
  int dc_table, ac_table;    // non-interleaved: Huffman table ids (0 / 1)
  long long interval;        // restart interval in blocks (interleaved: Ri * blocks per MCU), 0: none
  long long dri;             // the interval as the file states it (messages)
  long long offset, length;  // the entropy-coded segment, RSTm markers included
  long long nblocks;         // blocks the scan codes (interleaved: padding included)
  long long coef_off;        // non-interleaved: the component's first coefficient within the file
};
struct DecJobFile {
  bool interleaved;
  int n_scans;
  DecJobScan scan[3];
};

inline DecJobFile dec_jobs_of(const jds_jpeg_info* info) {
  DecJobFile f{};
  f.interleaved = info->interleaved != 0;
  f.n_scans = info->n_scans;
  if (f.interleaved) {  // (the block counts of hd_jpeg_mcu's record)
    const jds_jpeg_scan& s = info->scan[0];
    const long long bpm = info->blocks_per_mcu;
    f.scan[0] = {0, 0, s.restart_interval * bpm, s.restart_interval, s.offset, s.length,
                 bpm * info->mcu_cols * info->mcu_rows, 0};
    return f;
  }
  const long long yb = info->grid_cols[0] * info->grid_rows[0], cb = info->grid_cols[1] * info->grid_rows[1];
  for (int i = 0; i < info->n_scans; ++i) {  // (three; one for a grayscale file)
    const jds_jpeg_scan& s = info->scan[i];
    const int comp = s.component[0] - 1;
    f.scan[i] = {s.dc_table[0], s.ac_table[0], s.restart_interval, s.restart_interval, s.offset, s.length,
                 comp ? cb : yb, comp == 0 ? 0 : 64 * (yb + (comp - 1) * cb)};
  }
  return f;
}

enum DecJobsResult {
  DEC_JOBS_OK = 0,
  DEC_JOBS_UNSUPPORTED,  // a size beyond the descriptors' fields (the callers' JDS_ENOTSUP)
  DEC_JOBS_MARKERS       // restart markers missing from the scan data: a defective scan (JDS_EINVAL, or HD_RESTART)
};

// Appends the descriptors and lane intervals of a parsed file.  A scan without
// restart intervals is one descriptor of the self-synchronising kernels.  With
// an interval of at most lane_max blocks every interval goes to a lane of
// k_dec_rst; with a larger one every interval is a descriptor of its own (byte
// range, block count, destination), whose DC sum is the interval's.  On
// anything but DEC_JOBS_OK msg holds the reason (hd_walk's convention) and the
// vectors may hold part of the file's entries.
inline DecJobsResult dec_jobs_build(const uint8_t* data, const DecJobFile& file, const FilePlace& pl, int lane_max,
                                    std::vector<DecScan>& sc, std::vector<RstIv>& ivs, char* msg, size_t cap) {
  auto stop = [&](DecJobsResult r, const char* fmt, long long v) {
    (void)hd_fail(msg, cap, r, fmt, v);
    return r;
  };
  for (int i = 0; i < file.n_scans; ++i) {
    const DecJobScan& f = file.scan[i];
    if (f.length >= (int64_t)1 << 40) return stop(DEC_JOBS_UNSUPPORTED, "scan of %lld bytes", f.length);
    const long long nblocks = f.nblocks, ri = f.interval;
    if (nblocks > 0x7fffffffll) return stop(DEC_JOBS_UNSUPPORTED, "scan of %lld blocks", nblocks);
    const long long coef_off = pl.coef_off + f.coef_off;
    auto descriptor = [&](long long off, long long nbytes, long long blk0, long long nb) {
      DecScan d{};
      d.data_off = pl.data_off + off;
      d.nbytes = nbytes;
      d.nblocks = (int)nb;
      d.frame = pl.file;
      d.file = pl.file;
      if (file.interleaved) {  // (coef_off 0: the MCU record's off[] hold the file's place)
        d.dcs_off = pl.dcs_off;
        d.blk_base = (int)blk0;
      } else {
        d.coef_off = coef_off + 64 * blk0;
        d.dc_tab = 4 * pl.file + f.dc_table;
        d.ac_tab = 4 * pl.file + 2 + f.ac_table;
      }
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
        if (e - a > 0x7fffffffll) return stop(DEC_JOBS_UNSUPPORTED, "restart interval of %lld bytes", e - a);
        RstIv v{};
        v.data_off = pl.data_off + f.offset + a;
        v.coef_off = file.interleaved ? blk0 : coef_off + 64 * blk0;
        v.nbytes = (int)(e - a);
        v.nblk = (int)nb;
        v.frame = pl.file;
        v.file = pl.file;
        v.tabs = file.interleaved ? 0 : f.dc_table | ((2 + f.ac_table) << 8);
        ivs.push_back(v);
      } else {
        descriptor(f.offset + a, e - a, blk0, nb);
      }
      blk0 += nb;
      a = e + 2;
      if (e >= f.length && blk0 < nblocks)
        return stop(DEC_JOBS_MARKERS, "restart markers missing from the scan data (DRI %lld)", f.dri);
    }
  }
  return DEC_JOBS_OK;
}

}  // namespace jds
