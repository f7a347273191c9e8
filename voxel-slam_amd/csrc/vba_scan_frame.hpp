// What vba_scan.hip lets another unit see of a scan frame (the initialisation window of vba_init.hip reads stage 0 in place).
// Declarations only: struct vba_scan_frame lives in its unit.
#pragma once
#include "vba_ctx.hpp"

namespace vba {
// Stage 0 of a decoded frame (decoded, sorted, cut; vba_scan_prepare leaves it alone) for a reader on `stream`, which is ordered
// behind the decode.  false: the frame holds no decoded cloud.  stream == nullptr: the fields only, nothing is queued.
struct ScanStage0 { vba_ctx *ctx; int n; const double *pnt, *curv; };
bool scan_frame_stage0(vba_scan_frame *f, hipStream_t stream, ScanStage0 *out);
}  // namespace vba
