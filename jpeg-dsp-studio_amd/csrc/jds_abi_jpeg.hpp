// jds_abi_jpeg.hpp — what jds_abi_jpeg.hip (baseline files) shares with
// jds_abi_pjpeg.hip (progressive files): the argument checks of the renderings
// and the interleaved-scan writer's driver.  Defined in jds_abi_jpeg.hip.
// Private to csrc/.
#pragma once

#include <functional>
#include <vector>

#include "jds_abi.hpp"
#include "jds_entropy_mcu_dev.hpp"

// One file of a writer batch: its geometry record (the planes' offsets count
// from the start of c->ent_cf) and its header prefix.
struct McuJob {
  McuFile f;
  std::vector<uint8_t> pfx;
};

struct XfSet;

extern "C" {
int render_check(int32_t render);
int scale_check(int32_t render, int32_t denom);
// The launch arguments of a parsed file (tables, grids, chroma windows checked).
int jpeg_inv_args(const jds_jpeg_info* info, JInvArgs* a);
// The record of a parsed (or caller-filled) info whose planes start at coef_off.
int mcu_job_geo(const jds_jpeg_info* info, int64_t coef_off, McuJob* j);
// The writer over a batch's jobs, whose coefficients are in c->ent_cf (job k is
// item job_item[k]); jds_jpeg_batch_transcode's packing and item contract.
int mcu_write_batch(jds_ctx* c, std::vector<McuJob>& jobs, const std::vector<int>& job_item, int32_t optimize,
                    const XfSet* xf, uint8_t* out, int64_t out_cap, int32_t out_on_device,
                    jds_jpeg_transcode_item* items, int64_t* out_bytes,
                    const std::function<void(int, const char*)>& bad);
}
