// Floors for the fixed32 kernel on this MI355X: the memory floor (same loads/stores,
// trivial compute), the VALU floor (same hash, keys synthesised in registers, no loads),
// and the real kernel, timed interleaved in one process.  Also reports the in-kernel
// shader clock from s_memtime / s_memrealtime (100 MHz) in the VALU-floor kernel.
#include <hip/hip_runtime.h>
#include <cstdio>
#include <cstdint>
#include <cstdlib>
#include <vector>
#include <algorithm>
#include "../k2hash_amd/csrc/k2h_fnv_device.h"
#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); exit(1);} } while (0)
using namespace k2h;

__global__ __launch_bounds__(256) void k_mem(const uint4* __restrict__ keys, uint64_t n, uint64_t* __restrict__ h1) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint4 a = keys[2 * i], b = keys[2 * i + 1];
  h1[i] = ((uint64_t)(a.x ^ a.z ^ b.x ^ b.z) << 32) | (a.y ^ a.w ^ b.y ^ b.w);
}
__global__ __launch_bounds__(256) void k_alu(uint64_t n, uint64_t seed, uint64_t* __restrict__ h1, uint64_t* clk) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint64_t t0 = __builtin_amdgcn_s_memtime(), r0 = __builtin_amdgcn_s_memrealtime();
  uint32_t x = (uint32_t)i * 0x9E3779B9u;
  uint4 a = make_uint4(x, x ^ 0x55555555u, x + 7u, x * 3u), b = make_uint4(x ^ 1u, x + 11u, ~x, x ^ 0xABCDEFu);
  uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  fnv_chunk32(lo, hi, a, b);
  h1[i] = ((uint64_t)hi << 32) | lo;
  if (threadIdx.x == 0 && blockIdx.x % 1024 == 0) {
    uint64_t t1 = __builtin_amdgcn_s_memtime(), r1 = __builtin_amdgcn_s_memrealtime();
    clk[2 * (blockIdx.x / 1024)] = t1 - t0;
    clk[2 * (blockIdx.x / 1024) + 1] = r1 - r0;
  }
}
__global__ __launch_bounds__(256) void k_full(const uint4* __restrict__ keys, uint64_t n, uint64_t seed, uint64_t* __restrict__ h1) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint4 a = keys[2 * i], b = keys[2 * i + 1];
  uint32_t lo = (uint32_t)seed, hi = (uint32_t)(seed >> 32);
  fnv_chunk32(lo, hi, a, b);
  h1[i] = ((uint64_t)hi << 32) | lo;
}
// read-only floor: loads, no per-key store (one store per block)
__global__ __launch_bounds__(256) void k_read(const uint4* __restrict__ keys, uint64_t n, uint64_t* __restrict__ h1) {
  uint64_t i = (uint64_t)blockIdx.x * 256u + threadIdx.x;
  if (i >= n) return;
  uint4 a = keys[2 * i], b = keys[2 * i + 1];
  uint32_t v = a.x ^ a.y ^ a.z ^ a.w ^ b.x ^ b.y ^ b.z ^ b.w;
  if (v == 0x12345678u) h1[i] = v;
}
// Eight nt loads of a wave's four key rows, each a wave-uniform base + 32-bit lane offset +
// immediate (the base biased by 4 KiB so that the 13-bit signed immediate reaches every row).
typedef uint32_t v4u_q __attribute__((ext_vector_type(4)));
__device__ __forceinline__ void load_quad(const void* sbase, uint32_t voff, v4u_q (&x)[4], v4u_q (&y)[4]) {
  asm volatile("global_load_dwordx4 %0, %8, %9 offset:-4096 nt\n\t"
               "global_load_dwordx4 %1, %8, %9 offset:-4080 nt\n\t"
               "global_load_dwordx4 %2, %8, %9 offset:-2048 nt\n\t"
               "global_load_dwordx4 %3, %8, %9 offset:-2032 nt\n\t"
               "global_load_dwordx4 %4, %8, %9 offset:0 nt\n\t"
               "global_load_dwordx4 %5, %8, %9 offset:16 nt\n\t"
               "global_load_dwordx4 %6, %8, %9 offset:2048 nt\n\t"
               "global_load_dwordx4 %7, %8, %9 offset:2064 nt\n\t"
               "s_waitcnt vmcnt(0)"
               : "=&v"(x[0]), "=&v"(y[0]), "=&v"(x[1]), "=&v"(y[1]), "=&v"(x[2]), "=&v"(y[2]), "=&v"(x[3]), "=&v"(y[3])
               : "v"(voff), "s"(sbase)
               : "memory");
}
// The product's shape (fnv_fixed32_quad_kernel): one-wave blocks of 256 keys, four key rows
// per lane from a wave-uniform base, nt loads and stores; the memory floor of that shape
// (k_mem_quad) and the shipped four-key statement itself (k_full_quad).  n % 256 == 0 here.
__global__ __launch_bounds__(64) void k_mem_quad(const uint4* __restrict__ keys, uint64_t n, uint64_t* __restrict__ h1) {
  uint64_t* hb = h1 + (uint64_t)blockIdx.x * 256u;
  const uint32_t t = threadIdx.x;
  v4u_q x[4], y[4];
  load_quad(reinterpret_cast<const uint8_t*>(keys + (uint64_t)blockIdx.x * 512u) + 4096, t * 32u, x, y);
#pragma unroll
  for (int j = 0; j < 4; ++j)
    __builtin_nontemporal_store(((uint64_t)(x[j].x ^ x[j].z ^ y[j].x ^ y[j].z) << 32) | (x[j].y ^ x[j].w ^ y[j].y ^ y[j].w),
                                &hb[64 * j + t]);
}
__global__ __launch_bounds__(64) void k_full_quad(const uint4* __restrict__ keys, uint64_t n, uint64_t seed, uint64_t* __restrict__ h1) {
  const uint64_t first = (uint64_t)blockIdx.x * 256u;
  fnv_key32_quad_x<4>(threadIdx.x * 32u, (const uint8_t*)(keys + 2 * first) + 4096, threadIdx.x * 8u, h1 + first, seed);
}

int main() {
  const uint64_t n = 1ull << 24;
  uint4 *k0, *k1; uint64_t *h, *clk;
  CHK(hipMalloc(&k0, n * 32)); CHK(hipMalloc(&k1, n * 32)); CHK(hipMalloc(&h, n * 8)); CHK(hipMalloc(&clk, 64 * 8 * 2));
  CHK(hipMemset(k0, 0x5a, n * 32)); CHK(hipMemset(k1, 0xa5, n * 32));
  hipEvent_t e0, e1; CHK(hipEventCreate(&e0)); CHK(hipEventCreate(&e1));
  const unsigned g = (unsigned)(n / 256);
  const char* names[] = {"memory floor (load 32B, store 8B)", "read-only floor (load 32B)", "VALU floor (no loads)", "full fixed32 (flat)",
                         "memory floor, quad shape (nt, 64-thr)", "full fixed32, quad statement"};
  const int NV = 6;
  std::vector<float> t[NV];
  for (int r = 0; r < 7; ++r) {
    for (int v = 0; v < NV; ++v) {
      const int reps = 10;
      CHK(hipEventRecord(e0));
      for (int i = 0; i < reps; ++i) {
        const uint4* k = (i & 1) ? k1 : k0;
        if (v == 0) k_mem<<<g, 256>>>(k, n, h);
        else if (v == 1) k_read<<<g, 256>>>(k, n, h);
        else if (v == 2) k_alu<<<g, 256>>>(n, 14695981039346656037ULL, h, clk);
        else if (v == 3) k_full<<<g, 256>>>(k, n, 14695981039346656037ULL, h);
        else if (v == 4) k_mem_quad<<<g, 64>>>(k, n, h);
        else k_full_quad<<<g, 64>>>(k, n, 14695981039346656037ULL, h);
      }
      CHK(hipEventRecord(e1)); CHK(hipEventSynchronize(e1));
      float ms; CHK(hipEventElapsedTime(&ms, e0, e1));
      t[v].push_back(ms / reps);
    }
  }
  for (int v = 0; v < NV; ++v) {
    std::sort(t[v].begin(), t[v].end());
    double med = t[v][t[v].size() / 2];
    printf("%-40s median %8.2f us  min %8.2f us  -> %7.1f GB/s at 40 B/key (%.1f%% of 8 TB/s)\n", names[v], med * 1e3,
           t[v][0] * 1e3, 40.0 * n / (med * 1e-3) / 1e9, 100.0 * 40.0 * n / (med * 1e-3) / 8e12);
  }
  uint64_t hc[128]; CHK(hipMemcpy(hc, clk, sizeof hc, hipMemcpyDeviceToHost));
  double s = 0; int c = 0;
  for (int j = 0; j < 64; ++j) if (hc[2 * j + 1]) { s += (double)hc[2 * j] / (double)hc[2 * j + 1] * 0.1; ++c; }
  printf("in-kernel shader clock (VALU floor kernel, %d samples): %.3f GHz\n", c, c ? s / c : 0.0);
  return 0;
}
