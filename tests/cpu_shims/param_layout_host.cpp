// CPU shim for the host logic tests: the parameter tables and the flat-buffer offsets of rela_amd/csrc/param_layout.h
// (plain C++: the SAME functions the nets' loads and both learners call) behind a C ABI.  Built by
// tests/test_param_layout_host.py with g++.
// TEST INFRASTRUCTURE -- not part of the product library.
#include "../../rela_amd/csrc/param_layout.h"

using namespace rela_amd;

extern "C" {

// net: 0 = AtariFFNet, 1 = AtariLSTMNet.  cnt[nseg], off[nseg + 1] (room for kLstmNetSegs + 1 each); returns nseg
int shim_param_layout(int net, int A, long long* cnt, long long* off) {
  const int nseg = net == 0 ? kFFNetSegs : kLstmNetSegs;
  int64_t c[kLstmNetSegs], o[kLstmNetSegs + 1];
  if (net == 0) ffnet_param_counts(A, c);
  else lstmnet_param_counts(A, c);
  flat_offsets(c, nseg, o);
  for (int i = 0; i < nseg; ++i) cnt[i] = c[i];
  for (int i = 0; i <= nseg; ++i) off[i] = o[i];
  return nseg;
}
}
