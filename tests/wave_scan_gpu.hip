// vh_wave_incl_add / vh_wave_incl_max (viyadb_amd/csrc/vh_wave_scan.h) on the GPU against a host loop: one block of 256 threads, every wave
// scans its own 64 values. tests/test_gpu_wave_scan.py builds and runs this program (once as it stands, once with -DVH_WAVE_SCAN_SHFL=1).
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <vector>
#include "../viyadb_amd/csrc/vh_wave_scan.h"

#define BLOCK 256
enum { OP_ADD = 0, OP_MAX = 1, OP_ADD64 = 2, OP_ADD_IN_BRANCH = 3, OP_MAX_IN_BRANCH = 4 };

// in: BLOCK values per case (low words), hi: their high words (OP_ADD64); out: two words per value
__global__ __launch_bounds__(BLOCK) void wave_scan_cases(const uint32_t* in, const uint32_t* hi, const int* op, int ncases, uint32_t* out) {
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  for (int c = 0; c < ncases; ++c) {
    const uint32_t x = in[c * BLOCK + threadIdx.x], h = hi[c * BLOCK + threadIdx.x];
    unsigned long long r = 0;
    switch (op[c]) {                       // (op[c] is uniform: a scalar branch)
      case OP_ADD: r = vh_wave_incl_add(x); break;
      case OP_MAX: r = vh_wave_incl_max(x); break;
      case OP_ADD64: r = vh_wave_incl_add((unsigned long long)h << 32 | x); break;
      case OP_ADD_IN_BRANCH: if (wave & 1) r = vh_wave_incl_add(x); else r = 0xDEAD0000ull + threadIdx.x; break;      // waves 1 and 3 scan, 0 and 2 do not
      default: if (wave & 1) r = 0xBEEF0000ull + threadIdx.x; else r = vh_wave_incl_max(x); break;
    }
    out[2 * (c * BLOCK + threadIdx.x)] = (uint32_t)r;
    out[2 * (c * BLOCK + threadIdx.x) + 1] = (uint32_t)(r >> 32);
  }
}

#define CHECK(e) do { hipError_t err_ = (e); if (err_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #e, hipGetErrorString(err_)); return 2; } } while (0)

struct Case { const char* name; int op; std::vector<uint32_t> x, h; };

int main() {
  std::vector<Case> cases;
  auto add = [&](const char* name, int op, auto f) {
    Case c{name, op, std::vector<uint32_t>(BLOCK), std::vector<uint32_t>(BLOCK, 0u)};
    for (int i = 0; i < BLOCK; ++i) c.x[i] = f(i);
    cases.push_back(c);
  };
  uint64_t s = 0x9E3779B97F4A7C15ull;
  auto rnd = [&]() { s ^= s << 13; s ^= s >> 7; s ^= s << 17; return (uint32_t)(s >> 16); };
  for (int op : {OP_ADD, OP_MAX, OP_ADD_IN_BRANCH, OP_MAX_IN_BRANCH}) {
    add("zeros", op, [](int) { return 0u; });
    add("ones", op, [](int) { return 1u; });
    add("the lane number", op, [](int i) { return (uint32_t)(i & 63); });
    add("random 32-bit values (sums wrap)", op, [&](int) { return rnd(); });
  }
  add("packed halves, 32 per lane", OP_ADD, [](int i) { return (i & 63) < 32 ? 32u : 32u << 16; });
  add("packed halves, random counts up to 32", OP_ADD, [&](int i) { const uint32_t c = rnd() % 33u; return (i & 63) < 32 ? c : c << 16; });
  add("a marker in one slot", OP_MAX, [](int i) { return (i & 63) == 0 ? 1u : 0u; });
  add("markers in two slots", OP_MAX, [](int i) { return (i & 63) == 0 ? 7u : (i & 63) == 37 + (i >> 6) ? 8u : 0u; });
  add("markers in two slots, the second at a row's end", OP_MAX, [](int i) { return (i & 63) == 0 ? 1u : (i & 63) == 15 + 16 * (i >> 6) ? 2u : 0u; });
  add("markers in all 64 slots", OP_MAX, [](int i) { return (uint32_t)(i & 63) + 1u; });
  add("one marker in slot 63", OP_MAX, [](int i) { return (i & 63) == 63 ? 64u : 0u; });
  add("64-bit sums that carry into the high word", OP_ADD64, [&](int) { return 0xF0000000u | rnd(); });
  for (auto& h : cases.back().h) h = rnd();

  const int n = (int)cases.size();
  std::vector<uint32_t> in(n * BLOCK), hi(n * BLOCK), out(2 * n * BLOCK, 0xA5A5A5A5u);
  std::vector<int> op(n);
  for (int c = 0; c < n; ++c) {
    op[c] = cases[c].op;
    for (int i = 0; i < BLOCK; ++i) { in[c * BLOCK + i] = cases[c].x[i]; hi[c * BLOCK + i] = cases[c].h[i]; }
  }
  uint32_t *d_in, *d_hi, *d_out;
  int* d_op;
  CHECK(hipMalloc(&d_in, in.size() * 4)); CHECK(hipMalloc(&d_hi, hi.size() * 4)); CHECK(hipMalloc(&d_out, out.size() * 4)); CHECK(hipMalloc(&d_op, n * sizeof(int)));
  CHECK(hipMemcpy(d_in, in.data(), in.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_hi, hi.data(), hi.size() * 4, hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_op, op.data(), n * sizeof(int), hipMemcpyHostToDevice));
  CHECK(hipMemcpy(d_out, out.data(), out.size() * 4, hipMemcpyHostToDevice));
  hipLaunchKernelGGL(wave_scan_cases, dim3(1), dim3(BLOCK), 0, 0, d_in, d_hi, d_op, n, d_out);
  CHECK(hipGetLastError());
  CHECK(hipDeviceSynchronize());
  CHECK(hipMemcpy(out.data(), d_out, out.size() * 4, hipMemcpyDeviceToHost));

  int bad = 0;
  for (int c = 0; c < n; ++c) {
    for (int w = 0; w < BLOCK / 64; ++w) {
      unsigned long long acc = 0;
      for (int l = 0; l < 64; ++l) {
        const int i = w * 64 + l;
        const unsigned long long v = (unsigned long long)hi[c * BLOCK + i] << 32 | in[c * BLOCK + i];
        unsigned long long want;
        switch (op[c]) {
          case OP_ADD: acc = (uint32_t)(acc + (uint32_t)v); want = acc; break;
          case OP_MAX: acc = (uint32_t)v > acc ? (uint32_t)v : acc; want = acc; break;
          case OP_ADD64: acc += v; want = acc; break;
          case OP_ADD_IN_BRANCH: acc = (uint32_t)(acc + (uint32_t)v); want = (w & 1) ? acc : 0xDEAD0000ull + i; break;
          default: acc = (uint32_t)v > acc ? (uint32_t)v : acc; want = (w & 1) ? 0xBEEF0000ull + i : acc; break;
        }
        const unsigned long long got = (unsigned long long)out[2 * (c * BLOCK + i) + 1] << 32 | out[2 * (c * BLOCK + i)];
        if (got != want && bad++ < 20) fprintf(stderr, "case %d (%s, op %d) wave %d lane %d: got %llx, want %llx\n", c, cases[c].name, op[c], w, l, got, want);
      }
    }
  }
  if (bad) { fprintf(stderr, "%d mismatches\n", bad); return 1; }
  printf("wave scan ok: %d cases\n", n);
  return 0;
}
