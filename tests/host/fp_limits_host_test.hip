// Host-side driver for the raw-limb op table of tests/device/limit_ops.h (fields q, r, Fq2 and the G1 / G2 point ops): the SAME
// __host__ __device__ source the kernels compile, run on the CPU and driven by tests/test_limits_host.py against Python integers.
// Protocol (binary, uint32 words): stdin = batches [kind, op, n] + n input records; stdout = n output records per batch.
#include <cstdio>
#include <vector>

#include "../device/limit_ops.h"

using namespace gs;

int main() {
  uint32_t hdr[3];
  while (fread(hdr, 4, 3, stdin) == 3) {
    const int kind = (int)hdr[0], op = (int)hdr[1];
    const size_t n = hdr[2];
    if (kind < 0 || kind > 4) return 2;
    const size_t wi = limits::in_words(kind), wo = limits::out_words(kind);
    std::vector<uint32_t> in(n * wi), out(n * wo, 0u);
    if (fread(in.data(), 4, in.size(), stdin) != in.size()) return 3;
    for (size_t i = 0; i < n; ++i) limits::run_case(kind, op, in.data() + i * wi, out.data() + i * wo);
    if (fwrite(out.data(), 4, out.size(), stdout) != out.size()) return 4;
  }
  fflush(stdout);
  return 0;
}
