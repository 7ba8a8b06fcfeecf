// k2hash_amd -- device-side FNV-1a primitives for gfx950 (CDNA4).
//
// The reference hot loop (lib/k2hashfunc.cc:49-59) is, per key byte b,
//     h ^= (uint64_t)(int64_t)(signed char)b;   // sign-extended (lib/k2hashfunc.cc:53,55)
//     h *= 0x100000001b3;                        // 1099511628211 (lib/k2hashfunc.cc:56)
// with h seeded by 14695981039346656037 (lib/k2hashfunc.cc:51).
//
// On CDNA4 the 64-bit state lives in two VGPRs (lo, hi) and, with P = 2^40 + 435,
//     x_lo = lo ^ sext32(b)          x_hi = hi ^ sign(b)   (sign(b) = 0 or 0xffffffff)
//     h'   = x * P = x_lo*435 + ((x_hi*435 + (x_lo << 8)) << 32)
// which is five VALU ops per byte:
//     v_xor_b32_sdwa  x_lo, sext(w.BYTE_k), lo
//     v_xor_b32_sdwa  hi,   sext(u.BYTE_k), hi      u = per-byte sign smear of w (v_perm_b32)
//     v_mul_lo_u32    m, hi, 435
//     v_lshl_add_u32  t, x_lo, 8, m                  written into the odd half of a {0, t} pair
//     v_mad_u64_u32   {lo,hi}, x_lo, 435, {0, t}
// plus two ops per 4-byte word for the sign smear.  Measured on MI355X
// (tools/valu_rates*.hip, profiles/r01_valu_rates.txt) every one of these issues in
// ~4.2 cycles per wave64 per SIMD, so the mix is 5.5 slow-issue ops per byte.  hipcc's
// own lowering of the byte loop spends 6.5 (it materialises x_lo << 8 and uses v_add3).
//
// The {0, t} pair needs two adjacent physical VGPRs with the low one held at zero, which
// the compiler cannot be asked for through operand constraints, so the byte steps are
// written as asm statements over fixed physical registers: the chunk helpers bind the
// state, the zero half and the chunk words to them through "{vN}" operand constraints
// and declare the temporaries as clobbers (see K2H_X_STEP below), the whole-key and
// LDS-round statements name every register themselves.  The kernels stay within 64
// VGPRs, i.e. 8 waves/SIMD.  A portable C++ formulation (fnv_step_c) is kept for the
// byte tails.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace k2h {

constexpr uint64_t kSeedBuiltin = 14695981039346656037ULL;  // lib/k2hashfunc.cc:51
constexpr uint64_t kSeedStd = 2166136261ULL;                  // libstdc++ _Fnv_hash_impl default
constexpr uint64_t kPrime = 1099511628211ULL;                 // lib/k2hashfunc.cc:56
constexpr uint32_t kPrimeLo = 0x1b3u;                         // kPrime = 2^40 + 0x1b3
constexpr uint32_t kSmearSel = 0x090B080Au;                   // v_perm selector, see smear()
static_assert(kPrime == (1ull << 40) + kPrimeLo, "the split multiply's two halves");

// P^-1 mod 2^64 (P is odd, so invertible).  Newton: x *= 2 - P x doubles the correct low
// bits; P * P = 1 mod 8, so six rounds from x = P pass 64.
constexpr uint64_t prime_inverse() {
  uint64_t x = kPrime;
  for (int i = 0; i < 6; ++i) x *= 2 - kPrime * x;
  return x;
}
constexpr uint64_t kPrimeInverse = prime_inverse();
static_assert(kPrimeInverse * kPrime == 1, "P^-1 mod 2^64");

typedef uint32_t u32x4_ua __attribute__((ext_vector_type(4), aligned(1)));  // 16 bytes at any alignment

__device__ __forceinline__ uint64_t pack2(uint32_t lo, uint32_t hi) { return ((uint64_t)hi << 32) | lo; }

// Per-byte sign smear: byte k of the result is 0xff if byte k of w is >= 0x80, else 0.
// v_perm_b32 selectors 8..11 replicate the sign of bytes 1,3,5,7 of {src0:src1}; with
// src1 = w, src0 = w << 8 those are w.b1, w.b3, w.b0, w.b2.
__device__ __forceinline__ uint32_t smear(uint32_t w) {
  return __builtin_amdgcn_perm(w << 8, w, kSmearSel);
}

// Portable one-byte step on the split state (compiler-scheduled).
__device__ __forceinline__ void fnv_step_c(uint32_t& lo, uint32_t& hi, uint32_t byte) {
  int32_t sb = (int32_t)(int8_t)byte;
  uint32_t xlo = lo ^ (uint32_t)sb;
  uint32_t xhi = hi ^ (uint32_t)(sb >> 31);
  uint32_t t = xhi * kPrimeLo + (xlo << 8);
  uint64_t r = (uint64_t)xlo * kPrimeLo + ((uint64_t)t << 32);
  lo = (uint32_t)r;
  hi = (uint32_t)(r >> 32);
}

// ---------------------------------------------------------------------------
// Hand-scheduled chunk steps.  Registers:
//   v48 lo, v49 hi   state pair (mad64 destination)
//   v50 = 0, v51 = t the {0, t} addend pair
//   v52 x_lo, v53 m, v54 / v58 u (sign smears of a word pair), v[56:57] the pair << 8
// ---------------------------------------------------------------------------
#define K2H_X_STEP(W, U, K)                                                                            \
  "v_xor_b32_sdwa v52, sext(" W "), v48 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_" #K         \
  " src1_sel:DWORD\n\t"                                                                                \
  "v_xor_b32_sdwa v49, sext(" U "), v49 dst_sel:DWORD dst_unused:UNUSED_PAD src0_sel:BYTE_" #K          \
  " src1_sel:DWORD\n\t"                                                                                \
  "v_mul_lo_u32 v53, v49, %[p]\n\t"                                                                    \
  "v_lshl_add_u32 v51, v52, 8, v53\n\t"                                                                \
  "v_mad_u64_u32 v[48:49], vcc, v52, %[p], v[50:51]\n\t"
#define K2H_X_WORD(W, U) K2H_X_STEP(W, U, 0) K2H_X_STEP(W, U, 1) K2H_X_STEP(W, U, 2) K2H_X_STEP(W, U, 3)
#define K2H_X_SMEAR2(LO, HI, PAIR)                 \
  "v_lshlrev_b64 v[56:57], 8, " PAIR "\n\t"        \
  "v_perm_b32 v54, v56, " LO ", %[sel]\n\t"        \
  "v_perm_b32 v58, v57, " HI ", %[sel]\n\t"
#define K2H_X_PAIR(LO, HI, PAIR) K2H_X_SMEAR2(LO, HI, PAIR) K2H_X_WORD(LO, "v54") K2H_X_WORD(HI, "v58")
#define K2H_X_PAIR_LAST(LO, HI, PAIR)                                                                      \
  K2H_X_SMEAR2(LO, HI, PAIR) K2H_X_WORD(LO, "v54") K2H_X_STEP(HI, "v58", 0) K2H_X_STEP(HI, "v58", 1)        \
      K2H_X_STEP(HI, "v58", 2) "v_mov_b32 v60, v48\n\tv_mov_b32 v61, v49\n\t" K2H_X_STEP(HI, "v58", 3)

// The chunk helpers bind the state to v48/v49, the zero half of the addend pair to v50
// and the chunk words to v[40:43] (v[44:47] for the second chunk) through physical-
// register operand constraints ("{vN}"), so the allocator keeps the state in place from
// one statement to the next (no copies in or out of the window) and the words sit in
// adjacent pairs for the 64-bit-shift sign smear (K2H_X_SMEAR2).
#define K2H_P_CLOBBERS "v51", "v52", "v53", "v54", "v56", "v57", "v58", "vcc", "memory"

// 16 bytes (one uint4 chunk) into the state; BANK 1 takes the chunk in v[44:47]
// instead of v[40:43], so a loop that alternates banks (ping-pong) needs no copies.
template <int BANK = 0>
__device__ __forceinline__ void fnv_chunk16(uint32_t& lo, uint32_t& hi, uint4 c) {
  if constexpr (BANK == 0) {
    asm(K2H_X_PAIR("v40", "v41", "v[40:41]") K2H_X_PAIR("v42", "v43", "v[42:43]")
        : "+{v48}"(lo), "+{v49}"(hi)
        : "{v40}"(c.x), "{v41}"(c.y), "{v42}"(c.z), "{v43}"(c.w), "{v50}"(0u), [p] "s"(kPrimeLo),
          [sel] "s"(kSmearSel)
        : K2H_P_CLOBBERS);
  } else {
    asm(K2H_X_PAIR("v44", "v45", "v[44:45]") K2H_X_PAIR("v46", "v47", "v[46:47]")
        : "+{v48}"(lo), "+{v49}"(hi)
        : "{v44}"(c.x), "{v45}"(c.y), "{v46}"(c.z), "{v47}"(c.w), "{v50}"(0u), [p] "s"(kPrimeLo),
          [sel] "s"(kSmearSel)
        : K2H_P_CLOBBERS);
  }
}

// 32 bytes (two chunks), one statement.
__device__ __forceinline__ void fnv_chunk32(uint32_t& lo, uint32_t& hi, uint4 a, uint4 b) {
  asm(K2H_X_PAIR("v40", "v41", "v[40:41]") K2H_X_PAIR("v42", "v43", "v[42:43]")
          K2H_X_PAIR("v44", "v45", "v[44:45]") K2H_X_PAIR("v46", "v47", "v[46:47]")
      : "+{v48}"(lo), "+{v49}"(hi)
      : "{v40}"(a.x), "{v41}"(a.y), "{v42}"(a.z), "{v43}"(a.w), "{v44}"(b.x), "{v45}"(b.y), "{v46}"(b.z),
        "{v47}"(b.w), "{v50}"(0u), [p] "s"(kPrimeLo), [sel] "s"(kSmearSel)
      : K2H_P_CLOBBERS);
}

// Last 16-byte chunk of a key: also returns the state before the final byte
// (the reference's second hash, lib/k2hashfunc.cc:83-85).
__device__ __forceinline__ void fnv_chunk16_last(uint32_t& lo, uint32_t& hi, uint32_t& lo2, uint32_t& hi2, uint4 c) {
  asm(K2H_X_PAIR("v40", "v41", "v[40:41]") K2H_X_PAIR_LAST("v42", "v43", "v[42:43]")
      : "+{v48}"(lo), "+{v49}"(hi), "={v60}"(lo2), "={v61}"(hi2)
      : "{v40}"(c.x), "{v41}"(c.y), "{v42}"(c.z), "{v43}"(c.w), "{v50}"(0u), [p] "s"(kPrimeLo),
        [sel] "s"(kSmearSel)
      : K2H_P_CLOBBERS);
}

}  // namespace k2h

// ---------------------------------------------------------------------------
// Whole-key statement for 32-byte keys (fixed32 fast path): the two 16-byte loads, all
// 32 byte steps and the store in ONE asm statement over explicit registers, so that
//  - each pair of words gets its sign smear from one 64-bit shift + two v_perm_b32
//    (3 slow-issue ops per 8 bytes instead of 4), which needs the words in adjacent
//    registers -- something operand constraints cannot express;
//  - no moves in or out of the register window.
// Register window: v[40:47] key words, v48/v49 state, v50 = 0, v51 t, v52 x_lo,
// v53 m, v54/v58 smears, v[56:57] shifted pair, v[60:61] second-hash snapshot.
// ---------------------------------------------------------------------------
namespace k2h {

#define K2H_X_HEAD                                                     \
  "global_load_dwordx4 v[40:43], %[src], off nt\n\t"                   \
  "global_load_dwordx4 v[44:47], %[src], off offset:16 nt\n\t"         \
  "v_mov_b32 v48, %[slo]\n\t"                                          \
  "v_mov_b32 v49, %[shi]\n\t"                                          \
  "v_mov_b32 v50, 0\n\t"                                               \
  "s_waitcnt vmcnt(0)\n\t"
#define K2H_X_BODY                                                                                      \
  K2H_X_PAIR("v40", "v41", "v[40:41]") K2H_X_PAIR("v42", "v43", "v[42:43]") K2H_X_PAIR("v44", "v45", "v[44:45]")
#define K2H_X_CLOBBERS                                                                                   \
  "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v48", "v49", "v50", "v51", "v52", "v53", "v54", \
      "v55", "v56", "v57", "v58", "v59", "v60", "v61", "vcc", "memory"

// h1 only
__device__ __forceinline__ void fnv_key32_x(const void* src, uint64_t* dst1, uint64_t seed) {
  asm volatile(K2H_X_HEAD K2H_X_BODY K2H_X_PAIR("v46", "v47", "v[46:47]")
               "global_store_dwordx2 %[d1], v[48:49], off nt\n\t"
               "s_nop 1\n\t"
               :
               : [src] "v"(src), [d1] "v"(dst1), [slo] "s"((uint32_t)seed), [shi] "s"((uint32_t)(seed >> 32)),
                 [p] "s"(kPrimeLo), [sel] "s"(kSmearSel)
               : K2H_X_CLOBBERS);
}

// NK = 4 32-byte keys per lane, h1 only, as ONE statement over a wave's block of
// 64 NK keys: lane t hashes keys 64 j + t of the block, j < NK.  Every load and store is
// addressed as a wave-uniform SGPR base + one 32-bit lane offset + an immediate, so the
// only address VALU ops of the wave are the two lane offsets (voff = 32 t, doff = 8 t):
//   key j   at sbase - 4096 + 2048 j + voff   (sbase = the block's first key + 4096: the
//                                              13-bit signed immediate cannot reach +4096)
//   hash j  at dbase + 512 j + doff
// All 2 NK nt loads are issued first; key j is hashed in the registers it was loaded into
// as soon as its own two loads are in (vmcnt(2 (NK-1-j)); loads return in order), its hash
// parked in a spare pair while the next key runs, and all hashes stored at the end (a
// store among the loads would count in vmcnt out of order).  Registers: key 0 v[40:47],
// key 1 v[32:39], key 2 v[24:31], key 3 v[16:23]; window v48-v58 as above; parked hashes
// v[62:63], v[60:61], v[14:15], the last key's stays in v[48:49].  The caller guarantees
// that all 64 NK keys exist.
#define K2H_X_KEY(A, B, C, D, E, F, G, H)                                                           \
  K2H_X_PAIR("v" #A, "v" #B, "v[" #A ":" #B "]") K2H_X_PAIR("v" #C, "v" #D, "v[" #C ":" #D "]")     \
      K2H_X_PAIR("v" #E, "v" #F, "v[" #E ":" #F "]") K2H_X_PAIR("v" #G, "v" #H, "v[" #G ":" #H "]")
#define K2H_Q_LOAD(A, B, C, D, O0, O1)                                                  \
  "global_load_dwordx4 v[" #A ":" #B "], %[voff], %[sbase] offset:" #O0 " nt\n\t"       \
  "global_load_dwordx4 v[" #C ":" #D "], %[voff], %[sbase] offset:" #O1 " nt\n\t"
#define K2H_Q_SEED "v_mov_b32 v48, %[slo]\n\tv_mov_b32 v49, %[shi]\n\t"
#define K2H_Q_PARK(LO, HI, CNT) \
  "v_mov_b32 " LO ", v48\n\tv_mov_b32 " HI ", v49\n\t" K2H_Q_SEED "s_waitcnt vmcnt(" #CNT ")\n\t"
#define K2H_Q_STORE(PAIR, O) "global_store_dwordx2 %[doff], " PAIR ", %[dbase] offset:" #O " nt\n\t"
template <int NK>
__device__ __forceinline__ void fnv_key32_quad_x(uint32_t voff, const void* sbase, uint32_t doff, uint64_t* dbase,
                                                 uint64_t seed) {
  static_assert(NK == 4, "four keys per lane");
  asm volatile(K2H_Q_LOAD(40, 43, 44, 47, -4096, -4080) K2H_Q_LOAD(32, 35, 36, 39, -2048, -2032)
                   K2H_Q_LOAD(24, 27, 28, 31, 0, 16) K2H_Q_LOAD(16, 19, 20, 23, 2048, 2064)
                       K2H_Q_SEED "v_mov_b32 v50, 0\n\t"
               "s_waitcnt vmcnt(6)\n\t" K2H_X_KEY(40, 41, 42, 43, 44, 45, 46, 47)
               K2H_Q_PARK("v62", "v63", 4) K2H_X_KEY(32, 33, 34, 35, 36, 37, 38, 39)
               K2H_Q_PARK("v60", "v61", 2) K2H_X_KEY(24, 25, 26, 27, 28, 29, 30, 31)
               K2H_Q_PARK("v14", "v15", 0) K2H_X_KEY(16, 17, 18, 19, 20, 21, 22, 23)
               K2H_Q_STORE("v[62:63]", 0) K2H_Q_STORE("v[60:61]", 512) K2H_Q_STORE("v[14:15]", 1024)
               K2H_Q_STORE("v[48:49]", 1536) "s_nop 1\n\t"
               :
               : [voff] "v"(voff), [sbase] "s"(sbase), [doff] "v"(doff), [dbase] "s"(dbase), [slo] "s"((uint32_t)seed),
                 [shi] "s"((uint32_t)(seed >> 32)), [p] "s"(kPrimeLo), [sel] "s"(kSmearSel)
               : "v14", "v15", "v16", "v17", "v18", "v19", "v20", "v21", "v22", "v23", "v24", "v25", "v26", "v27",
                 "v28", "v29", "v30", "v31", "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", K2H_X_CLOBBERS,
                 "v62", "v63");
}

// Two 32-byte keys per lane as ONE statement: the four nt loads issued together (key 0
// into v[40:47], key 1 into v[32:39]), key 0 hashed as soon as ITS two loads have landed
// (vmcnt(2): loads return in order) while key 1's are still in flight, key 1 hashed in
// place (no copies into the window).  hipcc, given the loads as code, waited for all four
// before the first hash (vmcnt(0)).  The hashes are returned in registers (stored by the
// caller, e.g. with the fused bucket-index epilogue); H2 also returns each key's second hash
// (the state before its last byte: key 0's parked in v55/v59 while key 1 is hashed).
#define K2H_X_KEY1 \
  K2H_X_PAIR("v32", "v33", "v[32:33]") K2H_X_PAIR("v34", "v35", "v[34:35]") K2H_X_PAIR("v36", "v37", "v[36:37]") \
      K2H_X_PAIR("v38", "v39", "v[38:39]")
#define K2H_X_KEY1_LAST \
  K2H_X_PAIR("v32", "v33", "v[32:33]") K2H_X_PAIR("v34", "v35", "v[34:35]") K2H_X_PAIR("v36", "v37", "v[36:37]") \
      K2H_X_PAIR_LAST("v38", "v39", "v[38:39]")
#define K2H_PAIR_HEAD                                   \
  "global_load_dwordx4 v[40:43], %[s0], off nt\n\t"          \
  "global_load_dwordx4 v[44:47], %[s0], off offset:16 nt\n\t" \
  "global_load_dwordx4 v[32:35], %[s1], off nt\n\t"          \
  "global_load_dwordx4 v[36:39], %[s1], off offset:16 nt\n\t" \
  "v_mov_b32 v48, %[slo]\n\t"                                 \
  "v_mov_b32 v49, %[shi]\n\t"                                 \
  "v_mov_b32 v50, 0\n\t"                                      \
  "s_waitcnt vmcnt(2)\n\t"
#define K2H_PAIR_INPUTS                                                                                     \
  [s0] "v"(src0), [s1] "v"(src1), [slo] "s"((uint32_t)seed), [shi] "s"((uint32_t)(seed >> 32)), [p] "s"(kPrimeLo), \
      [sel] "s"(kSmearSel)
template <bool H2>
__device__ __forceinline__ void fnv_key32_pair_r(const void* src0, const void* src1, uint64_t seed, uint64_t& r0,
                                                 uint64_t& r1, uint64_t& s0, uint64_t& s1) {
  uint32_t a0, a1, b0, b1;
  if constexpr (!H2) {
    asm volatile(K2H_PAIR_HEAD K2H_X_BODY K2H_X_PAIR("v46", "v47", "v[46:47]")
                 "v_mov_b32 v62, v48\n\t"
                 "v_mov_b32 v63, v49\n\t"
                 "v_mov_b32 v48, %[slo]\n\t"
                 "v_mov_b32 v49, %[shi]\n\t"
                 "s_waitcnt vmcnt(0)\n\t" K2H_X_KEY1
                 : "={v62}"(a0), "={v63}"(a1), "={v48}"(b0), "={v49}"(b1)
                 : K2H_PAIR_INPUTS
                 : "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45",
                   "v46", "v47", "v50", "v51", "v52", "v53", "v54", "v55", "v56", "v57", "v58", "v59", "v60", "v61",
                   "vcc", "memory");
    s0 = s1 = 0;
  } else {
    uint32_t c0, c1, d0, d1;
    asm volatile(K2H_PAIR_HEAD K2H_X_BODY K2H_X_PAIR_LAST("v46", "v47", "v[46:47]")
                 "v_mov_b32 v62, v48\n\t"
                 "v_mov_b32 v63, v49\n\t"
                 "v_mov_b32 v55, v60\n\t"
                 "v_mov_b32 v59, v61\n\t"
                 "v_mov_b32 v48, %[slo]\n\t"
                 "v_mov_b32 v49, %[shi]\n\t"
                 "s_waitcnt vmcnt(0)\n\t" K2H_X_KEY1_LAST
                 : "={v62}"(a0), "={v63}"(a1), "={v48}"(b0), "={v49}"(b1), "={v55}"(c0), "={v59}"(c1),
                   "={v60}"(d0), "={v61}"(d1)
                 : K2H_PAIR_INPUTS
                 : "v32", "v33", "v34", "v35", "v36", "v37", "v38", "v39", "v40", "v41", "v42", "v43", "v44", "v45",
                   "v46", "v47", "v50", "v51", "v52", "v53", "v54", "v56", "v57", "v58", "vcc", "memory");
    s0 = pack2(c0, c1);
    s1 = pack2(d0, d1);
  }
  r0 = pack2(a0, a1);
  r1 = pack2(b0, b1);
}

}  // namespace k2h

// ---------------------------------------------------------------------------
// Eight 16-byte chunks read from LDS at per-lane addresses a[0..7] (one line of a key),
// hashed in order as ONE asm statement: reads alternate between v[40:43] and v[44:47],
// the next chunk's ds_read_b128 is in flight under the current chunk's steps, and the
// lgkmcnt waits are explicit -- the compiler's own wait insertion would otherwise
// treat every LDS read as aliasing the LDS-DMA loads still in flight and drain them
// all (s_waitcnt vmcnt(0)) before the first read.  The LDS slot is the ds_read immediate
// offset O (the per-lane addresses a[] stay fixed across rounds: no address VALU per
// round) and the zero half of the mad64 addend pair is carried in v50 by the caller (z,
// always 0; not re-materialised per statement).  _last: the eighth chunk is the key's
// final one and its pre-final-byte state (the second hash) is returned in lo2/hi2.
// ---------------------------------------------------------------------------
namespace k2h {

#define K2H_X_CHUNK_A K2H_X_PAIR("v40", "v41", "v[40:41]") K2H_X_PAIR("v42", "v43", "v[42:43]")
#define K2H_X_CHUNK_B K2H_X_PAIR("v44", "v45", "v[44:45]") K2H_X_PAIR("v46", "v47", "v[46:47]")
#define K2H_LAST_B K2H_X_PAIR("v44", "v45", "v[44:45]") K2H_X_PAIR_LAST("v46", "v47", "v[46:47]")
#define K2H_R8_CLOBBERS                                                                                      \
  "v40", "v41", "v42", "v43", "v44", "v45", "v46", "v47", "v51", "v52", "v53", "v54", "v56", "v57", "v58", "vcc", \
      "memory"
#define K2H_R8O_BODY(LASTCHUNK)                                              \
  "ds_read_b128 v[40:43], %[a0] offset:%[o]\n\t"                             \
  "ds_read_b128 v[44:47], %[a1] offset:%[o]\n\t"                             \
  "s_waitcnt lgkmcnt(1)\n\t" K2H_X_CHUNK_A                                   \
  "ds_read_b128 v[40:43], %[a2] offset:%[o]\n\t"                             \
  "s_waitcnt lgkmcnt(1)\n\t" K2H_X_CHUNK_B                                   \
  "ds_read_b128 v[44:47], %[a3] offset:%[o]\n\t"                             \
  "s_waitcnt lgkmcnt(1)\n\t" K2H_X_CHUNK_A                                   \
  "ds_read_b128 v[40:43], %[a4] offset:%[o]\n\t"                             \
  "s_waitcnt lgkmcnt(1)\n\t" K2H_X_CHUNK_B                                   \
  "ds_read_b128 v[44:47], %[a5] offset:%[o]\n\t"                             \
  "s_waitcnt lgkmcnt(1)\n\t" K2H_X_CHUNK_A                                   \
  "ds_read_b128 v[40:43], %[a6] offset:%[o]\n\t"                             \
  "s_waitcnt lgkmcnt(1)\n\t" K2H_X_CHUNK_B                                   \
  "ds_read_b128 v[44:47], %[a7] offset:%[o]\n\t"                             \
  "s_waitcnt lgkmcnt(1)\n\t" K2H_X_CHUNK_A                                   \
  "s_waitcnt lgkmcnt(0)\n\t" LASTCHUNK
#define K2H_R8O_INPUTS                                                                                       \
  [a0] "v"(a[0]), [a1] "v"(a[1]), [a2] "v"(a[2]), [a3] "v"(a[3]), [a4] "v"(a[4]), [a5] "v"(a[5]),              \
      [a6] "v"(a[6]), [a7] "v"(a[7]), [o] "n"(O), [p] "s"(kPrimeLo), [sel] "s"(kSmearSel)

template <int O>
__device__ __forceinline__ void fnv_lds_round8o(uint32_t& lo, uint32_t& hi, uint32_t& z, const uint32_t (&a)[8]) {
  asm volatile(K2H_R8O_BODY(K2H_X_CHUNK_B)
               : "+{v48}"(lo), "+{v49}"(hi), "+{v50}"(z)
               : K2H_R8O_INPUTS
               : K2H_R8_CLOBBERS);
}

template <int O>
__device__ __forceinline__ void fnv_lds_round8o_last(uint32_t& lo, uint32_t& hi, uint32_t& z, uint32_t& lo2,
                                                     uint32_t& hi2, const uint32_t (&a)[8]) {
  asm volatile(K2H_R8O_BODY(K2H_LAST_B)
               : "+{v48}"(lo), "+{v49}"(hi), "+{v50}"(z), "={v60}"(lo2), "={v61}"(hi2)
               : K2H_R8O_INPUTS
               : K2H_R8_CLOBBERS);
}

// One round of line DMA for the line kernel: 8 global_load_lds_dwordx4, each an SGPR base
// (`src`, wave-uniform) + the lane's 32-bit offset v[i], LDS destination m + 1024 i in M0.
// As asm, the compiler neither counts these loads nor waits for them: every wait on them
// is the caller's explicit s_waitcnt vmcnt.  M0 is compiler-reserved (it cannot be
// declared clobbered) and is not restored here: the caller's kernel must have no other M0
// user -- tests/test_kernel_source.py checks the line-DMA kernel's code for any.
#define K2H_DMA1(I, OFF)             \
  "s_add_u32 m0, %[m], " #OFF "\n\t" \
  "s_nop 0\n\t"                      \
  "global_load_lds_dwordx4 %[v" #I "], %[s]\n\t"
__device__ __forceinline__ void line_dma8(uint64_t src, uint32_t m, const uint32_t (&v)[8]) {
  asm volatile(K2H_DMA1(0, 0) K2H_DMA1(1, 0x400) K2H_DMA1(2, 0x800) K2H_DMA1(3, 0xc00) K2H_DMA1(4, 0x1000)
                   K2H_DMA1(5, 0x1400) K2H_DMA1(6, 0x1800) K2H_DMA1(7, 0x1c00)
               :
               : [s] "s"(src), [m] "s"(m), [v0] "v"(v[0]), [v1] "v"(v[1]), [v2] "v"(v[2]), [v3] "v"(v[3]),
                 [v4] "v"(v[4]), [v5] "v"(v[5]), [v6] "v"(v[6]), [v7] "v"(v[7])
               : "memory", "scc");
}
#undef K2H_DMA1

}  // namespace k2h
