// jds_abi_jpeg.hpp — what jds_abi_jpeg.hip (baseline files) shares with
// jds_abi_pjpeg.hip (progressive files): the argument checks of the renderings,
// the batch driver (layout, run, transcode tail) with the front end that says
// what differs between the two kinds of file, and the interleaved-scan writer's
// driver.  Defined in jds_abi_jpeg.hip.  Private to csrc/.
#pragma once

#include <functional>
#include <vector>

#include "jds_abi.hpp"
#include "jds_entropy_mcu_dev.hpp"
#include "jds_jpeg_ljs.hpp"

// One file of a writer batch: its geometry record (the planes' offsets count
// from the start of c->ent_cf) and its header prefix.
struct McuJob {
  McuFile f;
  std::vector<uint8_t> pfx;
};

struct XfSet;

// The failing item of a batch that jds_last_error names (batch_note): the one of the lowest index.
struct BatchBad {
  int first_bad = -1;
  char first_msg[400] = "";
  void bad(int i, const char* m) {
    if (first_bad < 0 || i < first_bad) {
      first_bad = i;
      snprintf(first_msg, sizeof first_msg, "%s", m);
    }
  }
};

// What the layout keeps per batch: the parsed frames, the inverse records of the
// files that take part (in batch order) and the tile maps of the four launches.
struct BatchPlan : BatchBad {
  std::vector<jds_jpeg_info> info;  // per file: its frame
  std::vector<int> rec_of;          // per file: its record, or -1
  std::vector<int> file_of;         // per record: its file
  std::vector<JInvRec> recs;
  std::vector<JInvMap> map[JI_MODES];          // the full-scale images
  std::vector<JInvMap> smap[JI_MODES][LS_ND];  // the scaled ones, per denominator 2, 4, 8
  bool any_scaled = false;
  std::vector<int> denom;  // per file: the denominator it is decoded at
  int64_t rgb_bytes = 0, coef_entries = 0;
  BatchPlan() {}
  // One parsed frame, for a run without the inverse (the single-file calls): no second parse and none
  // of the renderings' checks, so the record has no launch arguments and the maps are their sentinels.
  explicit BatchPlan(const jds_jpeg_info& frame)
      : info{frame}, rec_of{0}, file_of{0}, recs(1), denom{1}, coef_entries(frame.coeffs_needed) {
    for (std::vector<JInvMap>& m : map) m.assign(1, JInvMap{0, -1});
  }
};

// A run as its front end sees it.
struct BatchJob {
  jds_ctx* c;
  hipStream_t s;
  const BatchPlan& bp;
  const uint8_t* const* data;  // the caller's files, bp.file_of[k] the one of record k
  std::vector<size_t> foff;    // per record: its file's first byte in the file region
  long long files_bytes = 0;   // the file region's padded size, a multiple of 256; it starts the upload
  std::vector<uint32_t> st0;   // per record: its status word before the first launch (0 or HD_RESTART)
  // the run's one upload: sections appended, each at a 256-byte boundary
  struct Part {
    size_t off, bytes;
    const void* src;
  };
  std::vector<Part> parts;
  size_t total = 0;
  // -> the section's offset.  src stays the caller's until the run has staged it (null: reserved only).
  size_t add(const void* src, size_t bytes) {
    parts.push_back(Part{total, bytes, src});
    total = (total + bytes + 255) / 256 * 256;
    return parts.back().off;
  }
  template <class T>
  size_t add(const std::vector<T>& v) {
    return add(v.data(), sizeof(T) * v.size());
  }
  // describe says where the coefficients go (bp.coef_entries of them) and what the decode
  // wants zeroed in the stream behind the upload
  int16_t* cf_d = nullptr;
  void* zero_p = nullptr;
  size_t zero_n = 0;
  // for decode: the upload on the device and the status words in it
  char* dv = nullptr;
  uint32_t* st_d = nullptr;
  template <class T>
  const T* dev(size_t off) const {
    return (const T*)(dv + off);
  }
};

// What differs between a batch of baseline files and one of progressive files.
struct BatchFront {
  virtual ~BatchFront() {}
  // Layout, per file inside batch_parallel (a failure's message in this thread's g_err):
  // the file's frame; then, once the rendering takes the frame, what else must hold.
  virtual int parse(int i, const uint8_t* data, int64_t len, jds_jpeg_info* frame) = 0;
  virtual int check(int i, const jds_jpeg_info* frame) = 0;
  // Run, on the host: the decode's descriptors added to j, its scratch sized, j.cf_d (and j.st0, j.zero_*).
  virtual int describe(BatchJob& j) = 0;
  // Run, behind the upload: the decode launches.
  virtual int decode(BatchJob& j) = 0;
};

extern "C" {
int check_coef_cap(const int16_t* coeffs, int64_t cap, int64_t needed);
int render_check(int32_t render);
int scale_check(int32_t render, int32_t denom);
// The launch arguments of a parsed file (tables, grids, chroma windows checked).
int jpeg_inv_args(const jds_jpeg_info* info, JInvArgs* a);

// Parse every file, check what the single call checks before it decodes, and
// lay the outputs out: images JI_RGB_ALIGN apart at least, coefficients end to
// end.  A file that fails takes no space and does not stop the batch.
// draft (without denoms): {width, height} asked for; a file's denominator is
// then the largest of 8, 4, 2, 1 that is at most min(W / width, H / height).
int batch_layout(const uint8_t* const* data, const int64_t* lens, int32_t n, jds_jpeg_batch_item* items, BatchPlan& bp,
                 BatchFront& fe, int32_t render = JDS_RENDER_REFERENCE, const int32_t* denoms = nullptr,
                 jds_jpeg_scaled_item* scaled = nullptr, const int64_t* draft = nullptr);
// The first failing item by index ("file 3: ..."), where jds_last_error finds it.
void batch_note(const BatchBad& b, const char* what = "file");
// The launches of a laid-out batch with at least one record: one upload, the
// front end's decode (file k's coefficients at bp.recs[k].coef_off of j.cf_d),
// then with `inverse` the batch rendering into rgb; the status words into
// items.  Synchronous.  Without `inverse` rgb is not used.
// after (nullable): called with the device status words once the rendering is
// in the stream, for work that follows it there.
int batch_run(jds_ctx* c, BatchPlan& bp, BatchFront& fe, const uint8_t* const* data, const int64_t* lens, uint8_t* rgb,
              int32_t rgb_on_device, int16_t* coeffs, jds_jpeg_batch_item* items, bool inverse,
              int32_t render = JDS_RENDER_REFERENCE,
              const std::function<int(const uint32_t*, hipStream_t)>* after = nullptr);
// A batch of one as a single call's result: the item's error (batch_note's
// "file 0: <message>" -> the message), or its scan data's defect, is the call's.
int single_result(int item_rc, uint32_t status);
// Behind a run without the inverse: the transcode items from the batch's, the
// writer over the files that decoded (job_of(k, i, job): record k's, file i's
// geometry and header prefix; xf, nullable: the transformed files it adds to),
// and the note.
int batch_transcode_tail(jds_ctx* c, BatchPlan& bp, const std::vector<jds_jpeg_batch_item>& bi, int32_t n,
                         const std::function<int(size_t, int, McuJob*)>& job_of, const XfSet* xf, int32_t optimize,
                         uint8_t* out, int64_t out_cap, int32_t out_on_device, jds_jpeg_transcode_item* items,
                         int64_t* out_bytes);

// The record of a parsed (or caller-filled) info whose planes start at coef_off.
int mcu_job_geo(const jds_jpeg_info* info, int64_t coef_off, McuJob* j);
// The header prefix of a transcoded file: every segment before the first SOS except DHT and DRI.
int mcu_job_splice(const uint8_t* data, int64_t len, McuJob* j);
// The writer over a batch's jobs, whose coefficients are in c->ent_cf (job k is
// item job_item[k]); jds_jpeg_batch_transcode's packing (files at multiples of
// `align`, a power of two: 1 for a single call, whose *out_bytes is then its
// file's exact length) and item contract.
int mcu_write_batch(jds_ctx* c, std::vector<McuJob>& jobs, const std::vector<int>& job_item, int32_t optimize,
                    const XfSet* xf, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                    jds_jpeg_transcode_item* items, int64_t* out_bytes,
                    const std::function<void(int, const char*)>& bad, int64_t align = 256);
}
