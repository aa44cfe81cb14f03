/* libmphsir -- C ABI, gradient accumulation.  An addition to include/mphsir.h (its conventions hold: device pointers owned by the caller,
 * a call only enqueues work on `stream` and returns 0 or a negative MPHSIR_E* code without launching anything, capturable).  The surface
 * of mphsir.h itself is frozen by count (tests/test_cabi.py: its entry points, its structs, MPHSIR_K_COUNT), so an entry point added after
 * the freeze lives in a header of its own; mp-hsir_amd/_lib.py reads both with the same parser.
 */
#ifndef MPHSIR_ACCUM_H
#define MPHSIR_ACCUM_H
#include "mphsir.h"

#ifdef __cplusplus
extern "C" {
#endif

/* multi_accum: the accumulate form of the gradient hand-over -- gradient accumulation over K micro-batches per optimizer step
 * (mp-hsir_amd/engine.py DataParallelEngine(accum_steps=K); off unless the caller asks).  The table, the blocks and the row search are
 * mphsir_multi_copy's (rows {src pointer, dst pointer, n floats, first block} in DEVICE memory; a block moves up to 4096 floats);
 * 16-byte loads and stores where src and dst of a row are both 16-byte aligned, one float per lane otherwise, a tail that is no
 * multiple of 4 per element.  Per element, with m the micro index:
 *   m == 0:  dst = src          a plain store: dst is NOT read, whatever it held (a NaN included) is overwritten -- nothing is zero-filled
 *   m >= 1:  dst = dst + src    one fp32 addition (no multiply: nothing to fuse); NaN and +-inf propagate by IEEE rules
 * m = *micro_dev when micro_dev (optional DEVICE int32, read by the launch) is given -- `micro` is then ignored -- else `micro`: one
 * captured launch serves every micro-batch of a group (the precedent: ordinal_dev of mphsir_degrade_args).  The branch on m is uniform
 * over the grid.  Every dst element is touched by exactly one thread, no atomics: bitwise reproducible, independent of the geometry.
 * Launches under MPHSIR_K_MULTI_COPY, the hand-over's id (the launch timer reports the family, as the SSIM pair launches under the ids
 * of the spectral-loss pair): MPHSIR_K_COUNT stays.
 * Refused (MPHSIR_EINVAL, nothing launched): another struct_size; a null table_dev; nseg <= 0; total_blocks outside 1 .. 2^31 - 1; a
 * negative `micro` (also when micro_dev is given).  A negative *micro_dev cannot be refused by the host: the launch treats it as 0. */
typedef struct mphsir_multi_accum_args {
    uint32_t struct_size;       /* = sizeof(this struct), set by the caller: any other value is rejected with MPHSIR_EINVAL */
    const int64_t* table_dev;
    int32_t nseg;
    int64_t total_blocks;
    int32_t micro;
    const int32_t* micro_dev;
} mphsir_multi_accum_args;
int mphsir_multi_accum(const mphsir_multi_accum_args* a, void* stream);

#ifdef __cplusplus
}
#endif
#endif
