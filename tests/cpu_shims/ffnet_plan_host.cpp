// CPU shim for the host logic tests: the forward plan of rela_amd/csrc/ffnet.hip (ffnet_plan.h is plain C++: the SAME
// functions the library calls before it launches anything) behind a C ABI.  Built by tests/test_ffnet_plan_host.py
// with g++.
// TEST INFRASTRUCTURE -- not part of the product library.
#include "../../rela_amd/csrc/ffnet_plan.h"

using namespace rela_amd;

extern "C" {

// out: trunk, fc, keep_f32, unsplit_a3, fc_slices, fc_per, precision
void shim_plan_ffnet_forward(int mode, int net_precision, int N, int max_rows, int* out) {
  const FfnetPlan p = plan_ffnet_forward(mode, net_precision, N, max_rows);
  out[0] = p.trunk, out[1] = p.fc, out[2] = p.keep_f32, out[3] = p.unsplit_a3, out[4] = p.fc_slices, out[5] = p.fc_per;
  out[6] = p.precision;
}

// out: trunk, a3_records
void shim_plan_lstm_trunk(int fast, int emu, int has_rec_scratch, int N, int want_records, int* out) {
  const LstmTrunkPlan p = plan_lstm_trunk(fast != 0, emu != 0, has_rec_scratch != 0, N, want_records != 0);
  out[0] = p.trunk, out[1] = p.a3_records;
}

int shim_fc_bf16_slices(int N, int* per) { return fc_bf16_slices(N, per); }
int shim_fc_splits(int N) { return fc_splits(N); }
int shim_packs_bf16_fc(int max_rows) { return packs_bf16_fc(max_rows); }
int shim_learner_merged_rows(int B) { return learner_merged_rows(B); }

// the layouts a load of an AtariFFNet packs, those a plan's kernels read (bit = row of the layout table), and whether
// BfT is left to be packed on demand
unsigned shim_ffnet_pack_set(int max_rows, int precision, int on_device) { return ffnet_pack_set(max_rows, precision, on_device != 0); }
unsigned shim_ffnet_plan_reads(int mode, int net_precision, int N, int max_rows) {
  return ffnet_plan_reads(plan_ffnet_forward(mode, net_precision, N, max_rows));
}
int shim_ffnet_bft_on_demand(int max_rows, int precision, int on_device) {
  return ffnet_bft_on_demand(max_rows, precision, on_device != 0);
}
// the rows of the layout table an AtariFFNet holds, in the order tests/test_ffnet_plan_host.py names them; -> their number
int shim_ffnet_layouts(int* out) {
  const int rows[] = {kLayB1, kLayb1, kLayB2, kLayb2, kLayB3, kLayb3, kLayBh, kLaybh, kLayW1d, kLayB2f,
                      kLayB3f, kLayB2e, kLayB3e, kLayBf, kLayBfT, kLaybf, kLayBhp, kLayBff, kLayBfe};
  const int n = (int)(sizeof(rows) / sizeof(rows[0]));
  for (int i = 0; i < n; ++i) out[i] = rows[i];
  return n == kLayFFNetEnd ? n : -1;
}

// the thresholds, in the order tests/test_ffnet_plan_host.py names them
void shim_constants(long long* out) {
  out[0] = kFastMinN, out[1] = kFastTrunkMinN, out[2] = kEmuConvMinN, out[3] = kEmuFcMinN, out[4] = kEmuMaxN;
  out[5] = kFcSplitBelow, out[6] = kFcPartFloats, out[7] = kFcPartRows, out[8] = kFcPositions;
}
}
