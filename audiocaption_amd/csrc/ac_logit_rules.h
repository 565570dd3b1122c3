// Internal interface of the logit rules (csrc/logit_rules.hip), shared with the decode chain (csrc/decoder.hip).
#pragma once
#include "ac_common.h"
#include "../../include/audiocaption_hip.h"

// AC_OK, or AC_ERR_ARG for a rule set ac_logit_rules_apply refuses (host arithmetic only).
int ac_logit_rules_check(const ac_logit_rules* rules, int V);

// ac_logit_rules_apply as a step of an on-device search: `cnt` / `seg_rows` / `max_len` are the search's unfinished counts
// (csrc/decoder.hip struct Live) - the workgroup of a row whose segment had no unfinished row after step t - 1 returns before
// its first load, as every other launch of that step does.  cnt null: every row runs.
int ac_logit_rules_launch(const float* logit, long ld_in, float* out, long ld_out, int rows, int V, const int* tokens,
                          long ld_tok, int t, const ac_logit_rules* rules, const int* cnt, int seg_rows, int max_len,
                          hipStream_t s);
