/* poasta_amd_tb.h — the traceback walk of a dense one-piece run: the part of the C ABI of include/poasta_amd.h that says which
 * walk kernel ran and carries its override.  poasta_amd.h includes this file at its end, so a caller of that header has these
 * declarations; including this file alone gives the whole ABI as well.  Same library, same conventions. */
#ifndef POASTA_AMD_TB_H
#define POASTA_AMD_TB_H
#include "poasta_amd.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The separate traceback launch of a dense one-piece run has two kernels: the generic walk (every layout) and a lean one written
 * for u16 compact cells with the two Match-state flags in the score (POA_LAYOUT_DERIVED_GAPS, code_fmt 4), absolute encoding.  The
 * engine takes the lean kernel wherever it is eligible: POA_MODE_DENSE, a separate traceback launch, that layout, and planes of
 * fewer than 2^32 elements per query.  Same lanes per walk, same depth, same bytes out.
 * The override rides in tune[POA_TUNE_BAND_PAIR] (the table is full), above the two fields of POA_BAND_NARROW_SHIFT:
 * (value >> POA_TB_LEAN_SHIFT) & 3 = 0: the rule, 1: never the lean kernel, 2: wherever eligible (what the rule says today). */
#define POA_TB_LEAN_SHIFT 4
enum {
    POA_TB_KERNEL_NONE = 0,     /* no separate traceback launch (fused walk, or no dense one-piece pass) */
    POA_TB_KERNEL_GENERIC,      /* poa_traceback_kernel<cell, compact, lanes> */
    POA_TB_KERNEL_LEAN          /* poa_traceback_mf_kernel<lanes> */
};
/* the separate traceback launches of the dense pass of the last run: out[0] = POA_TB_KERNEL_* (LEAN only if every chunk ran
 * it, GENERIC if any chunk ran the generic kernel), out[1] = lanes per walk and out[2] = speculation depth of the last chunk,
 * out[3] = walks over all chunks.  All zero after a run of another family (two-piece, score-only, checkpointed).  A hybrid or
 * exact run reports the walk of its dense pass; the walk after the replay is always the generic kernel.  Host side only. */
int poa_batch_tb_info(poa_batch_t* b, uint32_t out[4]);

#ifdef __cplusplus
}
#endif
#endif /* POASTA_AMD_TB_H */
