"""Names under which the launch census (rela_prof_count_enable) reports the conv1 -> conv2 kernel of the split-bf16
mode: conv1 on the int8 matrix cores fused with conv2 through LDS (csrc/conv12_i8.h: conv12_i8; the half-frame bf16
generations were removed in r4)."""
CONV12 = "conv12_i8"
CONV12_JOBS = "conv12_i8_jobs"

# every kernel of the split-bf16 arithmetic (bf16x2 mode: two-part operands, int8 conv1) -- none of them may run in an
# f32x3 step, whose three-part kernels are listed per network
SPLIT_BF16 = frozenset({CONV12, CONV12_JOBS, "conv_bf16s<Conv3F>", "conv3_bf16s_jobs", "fc_bf16s", "fc_bf16s (split-K)",
                        "gemm_rec64_nt", "unsplit_records64", "unsplit_trunk_rows", "wgrad_conv1_bf16", "wgrad_conv2_bf16",
                        "wgrad_conv3_bf16", "dgrad_conv2_bf16", "dgrad_conv3_bf16"})
X3_FFNET = frozenset({"conv12_s3", "conv3_img_s3", "gemm_s3<fc>"})
X3_LSTM = frozenset({"conv12_s3", "conv3_img_s3", "gemm_s3<gates_x>"})

# The R2D2 learner's LSTM recurrence (csrc/learner_r2d2.hip): one persistent launch per half of the step, or one split-K
# GEMM + one cell kernel per time step (the two GEMMs are counted under "gemm_lds (f32)" as well, like every f32 GEMM).
# The per-step forward also launches R2D2_REC_ZERO once per net when there is a burn-in; the chains zero in the kernel.
R2D2_REC_CHAIN = {"lstm_rec_chain"}
R2D2_BPTT_CHAIN = {"lstm_bptt_chain"}
R2D2_REC_STEPS = {"gemm_lds<TileRec, ProbRecFwd>", "lstm_cell_fwd"}
R2D2_BPTT_STEPS = {"gemm_lds<TileRec, ProbRecBwd>", "lstm_cell_bwd"}
R2D2_REC_ZERO = "zero_hidden_where_terminal"
