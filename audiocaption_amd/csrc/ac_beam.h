// Internal interface of the beam search's per-clip merge (csrc/decoder.hip), shared with the ensemble search (csrc/ensemble.hip).
#pragma once
#include "ac_common.h"

// Per clip: the `beam` best of the nrows x beam per-row candidates cand_val / cand_idx [B * beam][beam] (nrows * beam <= 64;
// the lowest flattened index wins ties) -> top_val / top_idx [B][beam], the layout ac_trm_beam_update consumes.
int ac_beam_merge_launch(const float* cand_val, const int* cand_idx, int B, int beam, int nrows, float* top_val,
                         int* top_idx, hipStream_t s);
