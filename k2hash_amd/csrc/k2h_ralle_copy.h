// k2hash_amd -- the copy kernel of the calls that place their output by a scan of per-blob sizes
// (k2h_ralledata_unlink.hip, k2h_archive_apply.hip): the select copy kernel's scheme
// (k2h_ralledata_check.hip) over scanned places.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "k2h_endwalk.h"
#include "k2h_kernels.h"

namespace k2h {

// The select copy kernel (k2h_ralledata_check.hip) over scanned places: the tile's emitted blobs
// land back to back at out + place[first blob of the tile]; blob j of the tile holds span bytes
// [pre[j], pre[j + 1]); an unchanged blob's span byte x sits at blobs[x + delta[j]].  RW: chg[i]
// marks rewritten blobs (K2H_AMD_UNLINK_REWRITTEN); without it chg is not read.  A rewritten
// blob (rw[j]) has its span in the output and no source here: the rewrite kernel, which runs
// after this one, writes it.  Pieces wholly inside it are skipped; a piece it shares with other
// blobs is gathered and stored whole, with the rewritten blob's first source byte as filler.
template <bool RW, int BLOBS = 256, int TAB = 4096>
__global__ __launch_bounds__(BLOBS) void ralle_place_copy_kernel(const uint8_t* __restrict__ blobs,
                                                               const uint64_t* __restrict__ off, uint64_t n,
                                                               const uint64_t* __restrict__ place,
                                                               const uint32_t* __restrict__ rank,
                                                               const uint8_t* __restrict__ chg, uint8_t* __restrict__ out,
                                                               uint64_t* __restrict__ out_off,
                                                               uint64_t* __restrict__ index) {
  typedef uint32_t u32x4_al __attribute__((ext_vector_type(4)));
  __shared__ uint64_t pre[BLOBS + 1];
  __shared__ uint64_t delta[BLOBS];
  __shared__ uint8_t rw[BLOBS];
  __shared__ uint8_t tab[TAB];
  const uint32_t tid = threadIdx.x;
  const uint64_t r0 = (uint64_t)blockIdx.x * BLOBS, i = r0 + tid;
  const uint64_t D0 = place[r0];
  const uint64_t B = place[n - r0 < (uint64_t)BLOBS ? n : r0 + BLOBS] - D0;
  uint64_t x = B, len = 0, b = 0;
  uint32_t rewritten = 0;
  if (i < n) {
    const uint64_t at = place[i];
    const uint32_t rk = rank[i];
    x = at - D0;
    len = place[i + 1] - at;
    if (rank[i + 1] != rk) {
      b = off[i];
      if constexpr (RW) rewritten = chg[i] & K2H_AMD_UNLINK_REWRITTEN;
      out_off[rk] = at;
      if (index) index[rk] = i;
    }
  }
  pre[tid] = x;
  delta[tid] = b - x;
  if constexpr (RW) rw[tid] = (uint8_t)rewritten;
  auto is_rw = [&](uint32_t j) {
    if constexpr (RW) return rw[j] != 0;
    else return false;
  };
  if (tid == 0) pre[BLOBS] = B;
  if (blockIdx.x == 0 && tid == 0) out_off[rank[n]] = place[n];
  uint8_t* const dst = out + D0;
  const uint32_t a = (uint32_t)((uintptr_t)dst & 15u);
  const uint64_t npieces = (a + B + 15) >> 4;
  const bool tabled = npieces <= (uint64_t)TAB;  // block-uniform
  if (tabled && len) {
    const uint32_t last = (uint32_t)((x + len - 1 + a) >> 4);
    for (uint32_t p = x ? (uint32_t)((x + a + 15) >> 4) : 0u; p <= last; ++p) tab[p] = (uint8_t)tid;
  }
  __syncthreads();
  if (!B) return;
  for (uint64_t p = tid; p < npieces; p += BLOBS) {
    // the piece holds span bytes [x0, x0 + 16), this tile's part of it [xl, xh)
    const int64_t x0 = (int64_t)(16 * p) - (int64_t)a;
    const uint64_t xl = x0 < 0 ? 0 : (uint64_t)x0, xh = (uint64_t)(x0 + 16) < B ? (uint64_t)(x0 + 16) : B;
    uint32_t j = 0;  // the blob holding byte xl: the last j with pre[j] <= xl
    if (tabled) {
      j = tab[p];
    } else {
#pragma unroll
      for (uint32_t step = BLOBS / 2; step; step >>= 1)
        if (pre[j + step] <= xl) j += step;
    }
    if (is_rw(j) && pre[j + 1] >= xh) continue;  // wholly the rewrite kernel's
    const bool whole = xh - xl == 16;
    bool contiguous = whole && !is_rw(j);
    if (contiguous && pre[j + 1] < xh) {  // past blob j: every blob up to the one holding xh - 1
      for (uint32_t m = j; pre[m + 1] < xh;) {
        ++m;
        if (pre[m + 1] > pre[m] && (is_rw(m) || delta[m] != delta[j])) contiguous = false;
      }
    }
    if (contiguous) {
      const u32x4_ua w = *reinterpret_cast<const u32x4_ua*>(blobs + xl + delta[j]);
      *reinterpret_cast<u32x4_al*>(dst + x0) = u32x4_al{w.x, w.y, w.z, w.w};
      continue;
    }
    // eight places at a time, as the select copy: every place's source address, then the loads
    uint32_t w[4];
    uint32_t m = j;
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const uint8_t* src[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int64_t y = x0 + 8 * h + k;
        const uint64_t yc = y < (int64_t)xl ? xl : y >= (int64_t)xh ? xh - 1 : (uint64_t)y;
        while (pre[m + 1] <= yc) ++m;
        src[k] = blobs + (is_rw(m) ? pre[m] : yc) + delta[m];
      }
      uint32_t bt[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) bt[k] = *src[k];
      w[2 * h] = bt[0] | bt[1] << 8 | bt[2] << 16 | bt[3] << 24;
      w[2 * h + 1] = bt[4] | bt[5] << 8 | bt[6] << 16 | bt[7] << 24;
    }
    if (whole) {
      *reinterpret_cast<u32x4_al*>(dst + x0) = u32x4_al{w[0], w[1], w[2], w[3]};
    } else {
      for (uint64_t y = xl; y < xh; ++y) {
        const uint32_t k = (uint32_t)((int64_t)y - x0);
        dst[y] = (uint8_t)(w[k >> 2] >> (8 * (k & 3)));
      }
    }
  }
}

}  // namespace k2h
