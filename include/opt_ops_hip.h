/* opt_ops_hip.h -- C ABI of libopt_ops_hip.so: gradient-norm clipping and the AdamW update of a whole parameter list
 * as two gfx950 launches (torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW, decoupled weight decay, no amsgrad).
 * The same statement in torch ops, for CPU parameters: memotr_amd/optim.py (ClipAdamW); the cut of the work and the
 * traffic count: DESIGN.md, "Optimizer step".
 *
 * TABLES (device memory, built once by the caller; only the g column changes from step to step):
 *   tensors  optstep_tensor [n_tensors]  one row per parameter: p, g, m, v (float32, contiguous, numel elements each,
 *                                        any 4-byte alignment), numel, group.  g == NULL: the parameter has no gradient
 *                                        this step and nothing of it is read or written (p, m, v, step).
 *   chunks   optstep_chunk  [n_chunks]   one row per workgroup: elements [index * OPTSTEP_CHUNK, min(numel, (index + 1) *
 *                                        OPTSTEP_CHUNK)) of tensor `tensor`.  A tensor may span many chunks, a chunk
 *                                        never spans tensors.  Rows that point outside the tables are skipped.
 *   partials double [n_chunks]           sum of squares of each chunk's gradient (0 where g == NULL)
 *   steps    float  [n_tensors]          torch's per-parameter state["step"]; steps_prev: scratch of the same size
 *
 * optstep_sumsq: one workgroup per chunk; the squares (exact in float64) are added in float64 in a fixed order, no
 * atomics: the same inputs give the same bits.  The chunk-0 workgroup of a tensor also copies steps[t] to
 * steps_prev[t], so that the update kernel can advance steps[t] while other workgroups of the tensor still need the
 * old count.
 *
 * optstep_adamw: every workgroup first adds the partials in a fixed order in float64:
 *   total_norm = sqrt(sum),  coef = max_norm > 0 ? min(1, max_norm / (total_norm + 1e-6)) : 1      (NaN goes through)
 * (workgroup 0 stores float(total_norm) to *total_norm_out), then updates its chunk in float32 from the scalars
 *   step = steps_prev[t] + 1,  bc1 = 1 - b1^step,  bc2 = 1 - b2^step                               (float64)
 *   c = float(coef), d = float(1 - lr wd), w = float(1 - b1), b = float(b2), o = float(1 - b2),
 *   s = float(lr / bc1), q = float(sqrt(bc2)), e = float(eps)                                      (rounded once)
 * element by element, every operation rounded once, no approximate reciprocal or square root:
 *   gs = g c;  m' = m + w (gs - m);  v' = v b + (o gs) gs;  p' = p d - s (m' / (sqrt(v') / q + e))
 * The chunk-0 workgroup of a tensor with a gradient stores steps[t] = step.  g is never written.  16-byte loads and
 * stores where p, g, m and v of the tensor are all 16-byte aligned, 4-byte ones otherwise and for the last numel % 4
 * elements.  PRECONDITIONS: the tensors do not overlap; both calls of a step are issued on one stream, sumsq first.
 *
 * The hyper-parameters travel by value as kernel arguments (optstep_hyper is read on the host during the call).
 * Returns 0 or a non-zero code (optstep_last_error() has the text): 1 = bad argument (negative count, null pointer
 * with work to do, n_groups outside 1 .. OPTSTEP_MAX_GROUPS, a hyper-parameter torch.optim.AdamW refuses), 2 = a size
 * the 32-bit indexing does not cover, 3 = the launch failed.  Arguments are validated on the host without touching a
 * device; n_chunks == 0 is a successful no-op without a launch.  Launches on `stream` (hipStream_t as void*; NULL =
 * default stream) and does not synchronise.
 */
#ifndef OPT_OPS_HIP_H
#define OPT_OPS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OPTSTEP_ABI_VERSION 1
#define OPTSTEP_CHUNK 16384                     /* elements per chunk (one workgroup's unit of work) */
#define OPTSTEP_MAX_GROUPS 8
#define OPTSTEP_MAX_CHUNKS 1048576              /* 2^20 chunks = 2^34 elements */

typedef struct {                                /* 48 bytes */
    float *p;
    const float *g;
    float *m;
    float *v;
    int64_t numel;
    int32_t group;
    int32_t reserved;
} optstep_tensor;

typedef struct {                                /* 8 bytes */
    int32_t tensor;
    int32_t index;
} optstep_chunk;

typedef struct {
    double lr, weight_decay, beta1, beta2, eps;
} optstep_group;

typedef struct {
    optstep_group group[OPTSTEP_MAX_GROUPS];
} optstep_hyper;

int optstep_abi_version(void);
const char *optstep_last_error(void);

int optstep_sumsq(const optstep_tensor *tensors, const optstep_chunk *chunks, int n_tensors, int n_chunks,
                  double *partials, const float *steps, float *steps_prev, void *stream);

int optstep_adamw(const optstep_tensor *tensors, const optstep_chunk *chunks, int n_tensors, int n_chunks,
                  const double *partials, float *steps, const float *steps_prev, const optstep_hyper *hyper,
                  int n_groups, double max_norm, float *total_norm_out, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* OPT_OPS_HIP_H */
