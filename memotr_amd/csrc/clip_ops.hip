// clip_ops.hip -- libclip_ops_hip.so: the hand-written gfx950 kernels around the deformable-attention operator, for the
// clip train step and for the online tracker's device side (C ABI: include/clip_ops_hip.h).
//
// Most of the train step's launches come from here.  The small-tensor chains work on a few thousand elements, so their
// cost is the launch: one kernel per chain, straight-line fp32 code following the reference formulas (operation order
// kept where it is cheap to do so; `#pragma clang fp contract(off)` inside a function so that a product rounds before it
// is added, as in torch's separate kernels), fixed-order reductions where a sum is needed.  The larger kernels
// (attention, the MFMA linears, the track bank) are described in their headers.
//
// One translation unit; this file holds the two entry points that belong to no family.  Each header holds one family's
// kernels, in the anonymous namespace, and that family's extern "C" entry points, so that an argument check sits next
// to the kernel it protects:
//   clip_common.h      error text, launch(), the dynamic-LDS opt-in, box arithmetic, wave reductions, ballot ranks
//   clip_criterion.h   matching cost, pair box losses and IoU, focal loss, track ownership, focal labels, assignment
//   clip_handover.h    track hand-over between two frames, forward and backward
//   clip_boxes.h       sine embedding of the anchors, inverse sigmoid, box refinement
//   clip_rows.h        column sums, ReLU-backward column sums, residual add + LayerNorm, the backbone's shift + ReLU
//   clip_attention.h   multi-head self-attention over the decoder queries, forward and backward
//   clip_linear.h      the query-sized linears on fp32 MFMA, direct and LDS-staged
//   clip_tracks.h      result rows, track bank, bank result rows, draw table; the kept-track and the counters rule;
//                      CLEAR's match events and the error table; HOTA's match events, Identity's pairs, the
//                      per-identity association sums and the identity timeline
//   clip_fill_gaps.h   gap filling and short-track removal on a result table
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <atomic>

#include "../../include/clip_ops_hip.h"
#include "assign_core.h"
#include "clip_common.h"
#include "clip_criterion.h"
#include "clip_handover.h"
#include "clip_boxes.h"
#include "clip_rows.h"
#include "clip_attention.h"
#include "clip_linear.h"
#include "clip_tracks.h"
#include "clip_fill_gaps.h"

extern "C" {
int clipops_abi_version(void) { return CLIPOPS_ABI_VERSION; }

const char *clipops_last_error(void) { return g_err; }
}  // extern "C"
