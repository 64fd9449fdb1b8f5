// Stand-alone host check of mt3_notes_decode_traced (csrc/symbolic.cpp): random token streams through the plain and the
// traced entry point -- same notes, counts and total_time; every trace index inside the token buffer; an exactly sized
// notes / trace buffer is enough.  tests/test_note_trace.py builds it with symbolic.cpp and errors.cpp under
// -fsanitize=address,undefined and runs it: exit status 0 and "ok" mean no finding.
#include <cstdio>
#include <vector>
#include <random>
#include "mt3_hip.h"
int main() {
  mt3_codec c; mt3_build_codec(100, 10, 1, &c);
  int nc = mt3_codec_num_classes(&c);
  std::mt19937 g(1);
  for (int spec = 0; spec < 3; ++spec) for (int it = 0; it < 200; ++it) {
    int nseg = g() % 6; std::vector<int32_t> tok; std::vector<int64_t> off{0}; std::vector<double> st;
    for (int s = 0; s < nseg; ++s) { int n = g() % 300; for (int i = 0; i < n; ++i) tok.push_back((g() % 3) ? g() % 40 : (int)(g() % (nc + 10)) - 3); off.push_back(tok.size()); st.push_back(2.04 * ((s * 7) % 5)); }
    if (tok.empty()) tok.push_back(0);
    int64_t cap = tok.size() + 8, n1 = 0, n2 = 0, inv, drop; double tt1, tt2;
    std::vector<mt3_note> a(cap), b(cap); std::vector<int64_t> tr(cap * 2, -7);
    int r1 = mt3_notes_decode(&c, spec, nseg, tok.data(), off.data(), st.data(), nullptr, nullptr, a.data(), cap, &n1, &inv, &drop, &tt1);
    int r2 = mt3_notes_decode_traced(&c, spec, nseg, tok.data(), off.data(), st.data(), nullptr, nullptr, b.data(), cap, &n2, &inv, &drop, &tt2, tr.data());
    if (r1 || r2 || n1 != n2 || tt1 != tt2) { std::printf("mismatch\n"); return 1; }
    for (int64_t j = 0; j < n2; ++j) { if (tr[2*j] < 0 || tr[2*j] >= (int64_t)tok.size() || tr[2*j+1] < -1 || tr[2*j+1] >= (int64_t)tok.size()) { std::printf("bad index\n"); return 1; } }
    // exact capacity, and a NULL trace
    int r3 = mt3_notes_decode_traced(&c, spec, nseg, tok.data(), off.data(), st.data(), nullptr, nullptr, b.data(), n2, &n2, &inv, &drop, &tt2, tr.data());
    if (r3) { std::printf("exact capacity failed\n"); return 1; }
  }
  std::printf("ok\n"); return 0;
}
