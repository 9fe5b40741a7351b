// flvis_amd: batched pyramidal Lucas-Kanade tracker for gfx950 (CDNA4).
//
// Replaces cv::calcOpticalFlowPyrLK as the reference calls it:
//   temporal tracking   src/processing/lkorb_tracking.cpp:64-73   (31x31, maxLevel 10 -> clamped, 30 it, eps 1e-3, USE_INITIAL_FLOW)
//   stereo "matching"   src/processing/camera_frame.cpp:124-128   (same call, img0 -> img1, maxLevel 5 -> clamped)
//
// Mapping: ONE WAVE (64 lanes) per (stream, point); the wave walks the pyramid levels top-down and runs the <=30
// Gauss-Newton iterations in-kernel.  Lane l owns window row (l>>1) and the 16-column half (l&1) of the 31x31 window:
// the interpolated template (I, Ix, Iy as packed int16 pairs) lives in that lane's registers for the whole level.
// Scharr derivatives are computed on the fly from the staged source patch (no derivative image in HBM).
// The search image is cached per level as a 41-row x 52-byte REGION around the current position (window + 4 px margin,
// dword-aligned columns): iterations read their 32x32 window from LDS and only a move of more than the margin re-stages
// it -- no global load and no barrier in a steady-state iteration.  The bilinear interpolation + residual run on packed
// 16-bit pairs (v_perm_b32 to widen two bytes, v_dot2c_i32_i16 for the weights and for the b1/b2 accumulation): 6.5
// instructions per pixel.  Sums are exact integers (int32 per lane; the wave total is reduced as 16-bit halves with DPP
// row reductions + 4 readlanes) -> bit-exact vs the oracle.
// A steady-state Gauss-Newton iteration (no re-staging) is ~285 instructions of the temporal launch, ~355 before the
// cuts of profiles/r31_lk_diet.md (scripts/lk_isa_count.py prints the listing's counts): the point's positions are read
// through v_readfirstlane, so the position, range, region, convergence and oscillation tests are scalar branches with
// no exec-mask bookkeeping; a pixel pair is packed before it is shifted; all 64 lanes run the pixel loop.  What
// remains: 104 of the 285 are the 16 pixels' interpolation and residual, ~10 wait-state no-ops among them, 37 the wave
// sum, ~25 the weights and the LDS reads with their alignment, ~45 the update with the double-precision exit tests, ~35
// scalar tests and loop bookkeeping.
// A level's set-up, outside the iteration loop (profiles/r32_lk_level_setup.md): everything a wave needs of a pyramid level
// is one 64-byte descriptor (LKLevel, made on the host from the caller's PyrSel: adjacent scalar loads and one wait instead
// of a dependent load per field); the level scale 2^-level is built from its bits; both staging fast paths keep one lane ->
// (row, dword) map for the whole kernel (a block of rows per trip: the scalar base advances, the lane's offset and LDS
// address stay); and a cached level hands the temporal launch the floats the stereo launch computed from the Hessian sums
// (A11, A12, A22, D, minEig, 1 / D) instead of the sums.
#include "dev_common.hpp"
#include "img_kernels.hpp"

namespace flvis {

constexpr int LK_WIN = 31;
constexpr int LK_PS = 40;     // template-source patch row stride (bytes); 36 used
constexpr int LK_PROWS = 34;  // rows of the template-source patch
constexpr int LK_RM = 4;      // search-region margin (pixels)
constexpr int LK_RS = 52;     // search-region row stride (bytes): 13 dwords (odd -> conflict-free row walks)
constexpr int LK_RROWS = 33 + 2 * LK_RM;
// template cache (LKParams::tc): one slot per (stream, point); LK_TC_HDR header dwords -- position bits (2), tag (2), mask of the levels
// stored (1), the rest unused -- followed by LK_TC_LVL dwords per level: the 24 template registers (tI, tX, tY: 8 packed pairs each) of
// the 64 lanes as six 1 KB rows (one dwordx4 per lane and row); lane 63, which holds no template (window row 31), carries in its first
// six dwords the level's floats as the stereo launch computed them from the three Hessian sums: A11, A12, A22, D = A11 A22 - A12^2, minEig
// and 1 / D (computed only for a level that passes the stereo launch's tests, 0 otherwise) -- the temporal launch applies its own thresholds
// to minEig and D and takes the rest as it is: the same IEEE operations on the same sums, done once instead of once per launch.  Both
// launches get min_eig from one place (Frame::lk_params): a reader with a LOWER threshold than the writer's would pass a level whose 1 / D
// was never computed
constexpr int LK_TC_HDR = 64;
constexpr int LK_TC_LVL = 64 * 24;

typedef short lk_s2 __attribute__((ext_vector_type(2)));
typedef __attribute__((address_space(1))) uint32_t lk_gu32;  // a dword in global memory (global_load instead of flat_load)
typedef uint32_t lk_u4 __attribute__((ext_vector_type(4)));  // (a native vector: the non-temporal builtins do not take HIP's uint4 class)
// (by value: __builtin_bit_cast applied directly to a vector-element expression such as q.y reads element 0 with this compiler)
__device__ __forceinline__ lk_s2 lk_as_s2(uint32_t v) { return __builtin_bit_cast(lk_s2, v); }
// a float that is the same in every lane, said so to the compiler (v_readfirstlane_b32 of its bits)
__device__ __forceinline__ float lk_uniform(float v) {
  return __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, v)));
}
__device__ __forceinline__ long long lk_uniform64(long long v) {
  const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(v >> 32));
  return (long long)(((unsigned long long)hi << 32) | lo);
}
typedef unsigned short lk_u2 __attribute__((ext_vector_type(2)));
// (a1 >> S, a0 >> S) as a pair of 16-bit lanes for 8 <= S <= 16 and 0 <= a0, a1 < 2^24: bytes 1 and 2 of both (one v_perm_b32), then ONE
// packed logical shift by S - 8 instead of a shift per value before the pack
template <int S>
__device__ __forceinline__ lk_s2 lk_pack_shr(int a0, int a1) {
  static_assert(S >= 8 && S <= 16, "bytes 1 and 2 hold bits 8 .. 23");
  const lk_u2 p = __builtin_bit_cast(lk_u2, __builtin_amdgcn_perm((uint32_t)a1, (uint32_t)a0, 0x06050201u));
  return __builtin_bit_cast(lk_s2, (lk_u2)(p >> (unsigned short)(S - 8)));
}

// patch[r][c] = img(X0 + c, Y0 + r) for r < nrows, c < 36, REFLECT_101 outside the image.  Item 9 r + k is dword k of row r.  When the
// whole patch lies inside the image (wave-uniform test; nearly every point) there is nothing to reflect and nothing to divide: a trip is a
// block of 7 rows x 9 dwords on lanes 0 .. 62, and lane = 9 r + k keeps its (r, k) for the whole kernel -- the address of a load is a
// uniform base that advances by 7 rows per trip + the lane's 32-bit offset, the LDS address the lane's own + a constant of the trip.
// (bx, by) = the level's physical REFLECT_101 border: the fast path covers every block that lies inside the bordered storage.
__device__ __forceinline__ bool lk_load_patch(const uint8_t* __restrict__ img, int w, int h, int pitch, int bx, int by, int X0, int Y0,
                                              int nrows, uint8_t* patch) {
  if (X0 >= -bx && Y0 >= -by && X0 + 39 < w + bx && Y0 + nrows <= h + by) {  // (+ 39: the second dword of the last item stays inside the row)
    // ALL loads of the lane are issued before the first one is consumed: one memory round trip for the patch instead of one per trip
    // (the loop form waited for every load before it issued the next -- five dependent round trips of ~1 us under load)
    const __attribute__((address_space(1))) uint8_t* const base =
        (const __attribute__((address_space(1))) uint8_t*)(img + (ptrdiff_t)Y0 * pitch + (X0 & ~3));
    const int sh = X0 & 3;
    static_assert(LK_PROWS <= 5 * 7 && LK_PROWS > 4 * 7, "five trips, and the last one starts on a row of the patch");
    const int lane = (int)threadIdx.x, r = lane / 9, k = lane - 9 * r;
    const unsigned off = lane < 63 ? (unsigned)(r * pitch + 4 * k) : 0u;
    uint32_t lo[5], hi[5];
#pragma unroll
    for (int t = 0; t < 5; t++) {
      const bool on = lane < 63 && 7 * t + r < nrows;
      // (a lane past the end re-reads item 0 of the trip's block, row 7 t of the patch: never stored, and in bounds for nrows > 28 -- the
      // rows the fast-path test has checked; the only caller passes LK_PROWS)
      const unsigned o = on ? off : 0u;
      const __attribute__((address_space(1))) uint8_t* const bt = base + (ptrdiff_t)(7 * t) * pitch;
      lo[t] = *(const lk_gu32*)(bt + o);
      hi[t] = *(const lk_gu32*)(bt + o + 4);
    }
    // (every loaded value is "used" here, so the compiler cannot sink the last, predicated trip's loads behind the wait for the others; in
    // ONE statement: the compiler waits for each statement's operands with an s_waitcnt of its own)
    asm volatile("" : "+v"(lo[0]), "+v"(hi[0]), "+v"(lo[1]), "+v"(hi[1]), "+v"(lo[2]), "+v"(hi[2]), "+v"(lo[3]), "+v"(hi[3]), "+v"(lo[4]), "+v"(hi[4]));
    uint8_t* const dst = patch + r * LK_PS + 4 * k;
#pragma unroll
    for (int t = 0; t < 5; t++)
      if (lane < 63 && 7 * t + r < nrows) *reinterpret_cast<uint32_t*>(dst + 7 * LK_PS * t) = __builtin_amdgcn_alignbyte(hi[t], lo[t], sh);
    return false;
  }
  for (int i = threadIdx.x; i < nrows * 9; i += 64) {
    int r = i / 9, k = i - r * 9;
    int Y = Y0 + r, X = X0 + 4 * k;
    uint32_t v;
    if (Y >= 0 && Y < h && X >= 0 && X + 3 < w) {
      const uint8_t* row = img + (size_t)Y * pitch;
      int a = X & ~3, sh = X & 3;
      uint32_t lo = *reinterpret_cast<const uint32_t*>(row + a);
      uint32_t hi = sh ? *reinterpret_cast<const uint32_t*>(row + a + 4) : 0u;
      v = __builtin_amdgcn_alignbyte(hi, lo, sh);
    } else {
      const uint8_t* row = img + (size_t)reflect101c(Y, h) * pitch;
      uint32_t b0 = row[reflect101c(X, w)], b1 = row[reflect101c(X + 1, w)], b2 = row[reflect101c(X + 2, w)],
               b3 = row[reflect101c(X + 3, w)];
      v = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
    *reinterpret_cast<uint32_t*>(patch + r * LK_PS + 4 * k) = v;
  }
  return true;
}

// region[r][c] = img(X0 + c, Y0 + r), r < LK_RROWS, c < 52, X0 a multiple of 4 (aligned dword loads), REFLECT_101 outside.  Same fast
// path when the region lies inside the image: a trip is a block of 4 rows x 13 dwords on lanes 0 .. 51 (lane = 13 r + k: the block is
// contiguous in LDS, item at byte 4 lane), eleven trips, the last one of a single row.  Two loads more than 64 items per trip would
// take, and no address arithmetic on the vector unit but the lane's own offset.
__device__ __forceinline__ bool lk_load_region(const uint8_t* __restrict__ img, int w, int h, int pitch, int bx, int by, int X0, int Y0,
                                               uint8_t* region) {
  if (X0 >= -bx && Y0 >= -by && X0 + 51 < w + bx && Y0 + LK_RROWS <= h + by) {
    // all loads of the lane in flight at once, then the LDS stores (see lk_load_patch)
    const __attribute__((address_space(1))) uint8_t* const base = (const __attribute__((address_space(1))) uint8_t*)(img + (ptrdiff_t)Y0 * pitch + X0);
    static_assert(LK_RS == 52, "the region rows are contiguous in LDS: a block of four rows is 52 dwords");
    constexpr int T = (LK_RROWS + 3) / 4, LAST = (LK_RROWS - 4 * (T - 1)) * 13;  // (lanes of the last trip)
    const int lane = (int)threadIdx.x, r = lane / 13, k = lane - 13 * r;
    const unsigned off = lane < 52 ? (unsigned)(r * pitch + 4 * k) : 0u;  // (an idle lane re-reads item 0 of the block: in bounds, never stored)
    uint32_t v[T];
#pragma unroll
    for (int t = 0; t < T; t++) v[t] = *(const lk_gu32*)(base + (ptrdiff_t)(4 * t) * pitch + (t < T - 1 || lane < LAST ? off : 0u));
    // (every loaded value is "used" in ONE statement: the compiler waits for each statement's operands with an s_waitcnt of its own)
    static_assert(T == 11, "the operand list below");
    asm volatile("" : "+v"(v[0]), "+v"(v[1]), "+v"(v[2]), "+v"(v[3]), "+v"(v[4]), "+v"(v[5]), "+v"(v[6]), "+v"(v[7]), "+v"(v[8]), "+v"(v[9]),
                 "+v"(v[10]));
    if (lane < 52) {
#pragma unroll
      for (int t = 0; t < T - 1; t++) *reinterpret_cast<uint32_t*>(region + 4 * lane + 4 * LK_RS * t) = v[t];
      if (lane < LAST) *reinterpret_cast<uint32_t*>(region + 4 * lane + 4 * LK_RS * (T - 1)) = v[T - 1];
    }
    return false;
  }
  for (int i = threadIdx.x; i < LK_RROWS * 13; i += 64) {
    int r = i / 13, k = i - r * 13;
    int Y = Y0 + r, X = X0 + 4 * k;
    uint32_t v;
    if (Y >= 0 && Y < h && X >= 0 && X + 3 < w) {
      v = *reinterpret_cast<const uint32_t*>(img + (size_t)Y * pitch + X);
    } else {
      const uint8_t* row = img + (size_t)reflect101c(Y, h) * pitch;
      uint32_t b0 = row[reflect101c(X, w)], b1 = row[reflect101c(X + 1, w)], b2 = row[reflect101c(X + 2, w)],
               b3 = row[reflect101c(X + 3, w)];
      v = b0 | (b1 << 8) | (b2 << 16) | (b3 << 24);
    }
    *reinterpret_cast<uint32_t*>(region + r * LK_RS + 4 * k) = v;
  }
  return true;
}

// bytes K and K+1 of the dword array D, widened to a pair of 16-bit lanes (one v_perm_b32; K is a compile-time constant)
#define LK_PAIR(D, K)                                                                                              \
  ((((K)&3) == 3) ? __builtin_amdgcn_perm((D)[((K) >> 2) + 1], (D)[(K) >> 2], 0x0c040c03u)                         \
                  : __builtin_amdgcn_perm(0u, (D)[(K) >> 2], 0x0c000c00u | (uint32_t)((K)&3) | ((uint32_t)(((K)&3) + 1) << 16)))

// Instruction diet of the iteration (round 6; continued in profiles/r31_lk_diet.md).  The LK launches are bound by INSTRUCTION ISSUE -- one instruction of any kind per 4 cycles
// and SIMD, vector, scalar, LDS, wait and no-op alike (profiles/r06_chain_ab.md; SQ counters: 0.44 scalar instructions per vector one) --
// not by latency: what shortens them is fewer instructions per iteration (rounds 3-5's forms were measured against these there).
// a . b + c with c in a SCALAR register (v_dot2_i32_i16, the three-source form): the rounding bias of a bilinear interpolation is a
// constant, and the accumulate-in-place form the compiler picks for the builtin (v_dot2c_i32_i16) needs a v_mov of it per pixel
__device__ __forceinline__ int lk_dot2_bias(lk_s2 a, lk_s2 b, int bias_uniform) {
  int r;
  asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(r) : "v"(a), "v"(b), "s"(bias_uniform));
  return r;
}
// the exact wave totals of two per-lane int32 as floats, (float)(long long) of each (round to nearest even): the four 16-bit-half chains
// advance together, step by step (every DPP step's operands were written four instructions earlier: no wait states to fill), and the
// totals are put together in double -- hi * 65536 + lo is exact below 2^53, one rounding into float -- on the vector unit in lane 63
// instead of ~13 scalar instructions per value (count leading zeros, shift, sticky bit, convert, scale); two read-lanes instead of four
__device__ __forceinline__ void lk_wave_sum2_f32(int v1, int v2, float& f1, float& f2) {
  int a = v1 & 0xffff, b = v1 >> 16, c = v2 & 0xffff, d = v2 >> 16;
#define LK_STEP4(CTRL, RM)                                           \
  {                                                                  \
    const int ta = __builtin_amdgcn_update_dpp(0, a, CTRL, RM, 0xf, false); \
    const int tb = __builtin_amdgcn_update_dpp(0, b, CTRL, RM, 0xf, false); \
    const int tc = __builtin_amdgcn_update_dpp(0, c, CTRL, RM, 0xf, false); \
    const int td = __builtin_amdgcn_update_dpp(0, d, CTRL, RM, 0xf, false); \
    a += ta, b += tb, c += tc, d += td;                              \
  }
  LK_STEP4(0xB1, 0xf)   // quad_perm [1,0,3,2]
  LK_STEP4(0x4E, 0xf)   // quad_perm [2,3,0,1]
  LK_STEP4(0x141, 0xf)  // row_half_mirror
  LK_STEP4(0x140, 0xf)  // row_mirror
  LK_STEP4(0x142, 0xa)  // row_bcast:15, rows 1 and 3
  LK_STEP4(0x143, 0xc)  // row_bcast:31, rows 2 and 3
#undef LK_STEP4
  const float g1 = (float)__builtin_fma((double)b, 65536.0, (double)a), g2 = (float)__builtin_fma((double)d, 65536.0, (double)c);
  f1 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g1), 63));
  f2 = __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, g2), 63));
}

// the exact 64-bit wave totals of three per-lane int32 (the Hessian sums of a template level): six 16-bit-half chains advancing together
// -- a DPP step's operand was written six instructions earlier, so none of the ~30 wait-state no-ops of three reductions one after the
// other
__device__ __forceinline__ void lk_wave_sum3_wide(int v1, int v2, int v3, long long& s1, long long& s2, long long& s3) {
  int a = v1 & 0xffff, b = v1 >> 16, c = v2 & 0xffff, d = v2 >> 16, e = v3 & 0xffff, f = v3 >> 16;
#define LK_STEP6(CTRL, RM)                                                    \
  {                                                                           \
    const int ta = __builtin_amdgcn_update_dpp(0, a, CTRL, RM, 0xf, false);  \
    const int tb = __builtin_amdgcn_update_dpp(0, b, CTRL, RM, 0xf, false);  \
    const int tc = __builtin_amdgcn_update_dpp(0, c, CTRL, RM, 0xf, false);  \
    const int td = __builtin_amdgcn_update_dpp(0, d, CTRL, RM, 0xf, false);  \
    const int te = __builtin_amdgcn_update_dpp(0, e, CTRL, RM, 0xf, false);  \
    const int tf = __builtin_amdgcn_update_dpp(0, f, CTRL, RM, 0xf, false);  \
    a += ta, b += tb, c += tc, d += td, e += te, f += tf;                     \
  }
  LK_STEP6(0xB1, 0xf)
  LK_STEP6(0x4E, 0xf)
  LK_STEP6(0x141, 0xf)
  LK_STEP6(0x140, 0xf)
  LK_STEP6(0x142, 0xa)
  LK_STEP6(0x143, 0xc)
#undef LK_STEP6
  s1 = ((long long)__builtin_amdgcn_readlane(b, 63) << 16) + (long long)__builtin_amdgcn_readlane(a, 63);
  s2 = ((long long)__builtin_amdgcn_readlane(d, 63) << 16) + (long long)__builtin_amdgcn_readlane(c, 63);
  s3 = ((long long)__builtin_amdgcn_readlane(f, 63) << 16) + (long long)__builtin_amdgcn_readlane(e, 63);
}

// The interpolated template of one level: I, Ix, Iy of the 31 x 31 window as packed int16 pairs in the lane's registers (lane = window
// row lane >> 1, 16-column half lane & 1) and this lane's share of the three Hessian sums.  Packed 16-bit path: two columns per
// instruction (v_pk_*), the bilinear weights applied with v_dot2c_i32_i16.  Every lane (window rows 0 .. 31: the lanes of row 31 only
// serve their neighbours) computes the Scharr derivatives of ITS row once; the derivatives of row r + 1, which the bilinear
// interpolation also needs, come from the lane two above (same column half) through ds_bpermute -- 18 exchanges on the LDS pipe instead
// of computing every derivative row twice on the VALUs.  INTERIOR: every pixel the stencil is evaluated at lies inside the image.
// Otherwise the derivative image is ZERO outside the image (cv::calcOpticalFlowPyrLK's derivative pyramid has a constant border, the
// intensity pyramid a reflected one): the staged patch holds the reflected intensities, the derivatives of this lane's row are masked
// per column pair before they are used and exchanged (9 masks from one 18-bit column-validity word).
template <bool INTERIOR>
__device__ __forceinline__ void lk_template(const uint8_t* patch, int lane, int ipx, int ipy, int W, int H, lk_s2 wT, lk_s2 wB,
                                            lk_s2 (&tI)[8], lk_s2 (&tX)[8], lk_s2 (&tY)[8], int& a11, int& a12, int& a22) {
  constexpr int W_BITS = 14;
  const int r = lane >> 1, c0 = (lane & 1) * 16;
  uint32_t d[3][5];
#pragma unroll
  for (int j = 0; j < 3; j++)
#pragma unroll
    for (int k = 0; k < 5; k++) d[j][k] = *reinterpret_cast<const uint32_t*>(patch + (r + j) * LK_PS + c0 + 4 * k);
  uint32_t bits = 0;
  if (!INTERIOR) {
    // window columns c0 .. c0 + 17 of this lane's row: image (ipx + c0 + c, ipy + r)
    const int xs = ipx + c0, Y = ipy + r;
    int lo = -xs, hi = W - xs;
    lo = lo < 0 ? 0 : (lo > 18 ? 18 : lo);
    hi = hi < 0 ? 0 : (hi > 18 ? 18 : hi);
    bits = (Y >= 0 && Y < H && hi > lo) ? (((1u << hi) - 1u) & ~((1u << lo) - 1u)) : 0u;
  }
  lk_s2 DX[2][9], DY[2][9];  // (v[2j], v[2j+1]) of window row r + dr
  {
    lk_s2 T0[10], T1[10];
#pragma unroll
    for (int j = 0; j < 10; j++) {
      const lk_s2 A = __builtin_bit_cast(lk_s2, LK_PAIR(d[0], 2 * j)), B = __builtin_bit_cast(lk_s2, LK_PAIR(d[1], 2 * j)),
                  Cc = __builtin_bit_cast(lk_s2, LK_PAIR(d[2], 2 * j));
      T0[j] = (A + Cc) * (short)3 + B * (short)10;
      T1[j] = Cc - A;
    }
    const int up2 = ((lane + 2) & 63) * 4;
#pragma unroll
    for (int j = 0; j < 9; j++) {
      DX[0][j] = T0[j + 1] - T0[j];
      const lk_s2 T1o = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, T1[j + 1]),
                                                                       __builtin_bit_cast(uint32_t, T1[j]), 0x05040302u));
      DY[0][j] = (T1[j + 1] + T1[j]) * (short)3 + T1o * (short)10;
      if (!INTERIOR) {
        const uint32_t m = ((bits >> (2 * j)) & 1u ? 0x0000ffffu : 0u) | ((bits >> (2 * j + 1)) & 1u ? 0xffff0000u : 0u);
        DX[0][j] = __builtin_bit_cast(lk_s2, __builtin_bit_cast(uint32_t, DX[0][j]) & m);
        DY[0][j] = __builtin_bit_cast(lk_s2, __builtin_bit_cast(uint32_t, DY[0][j]) & m);
      }
      DX[1][j] = __builtin_bit_cast(lk_s2, __builtin_amdgcn_ds_bpermute(up2, __builtin_bit_cast(int, DX[0][j])));
      DY[1][j] = __builtin_bit_cast(lk_s2, __builtin_amdgcn_ds_bpermute(up2, __builtin_bit_cast(int, DY[0][j])));
    }
  }
  if (r < LK_WIN) {
    // (intensity rows r, r + 1 of the window are patch rows r + 1, r + 2: d[1], d[2])
#pragma unroll
    for (int c2 = 0; c2 < 8; c2++) {
      int iv[2], ix[2], iy[2];
#pragma unroll
      for (int hh = 0; hh < 2; hh++) {
        const int c = 2 * c2 + hh;
        lk_s2 x0, x1, y0, y1;  // (v[c], v[c+1]) of rows r, r+1
        if (hh == 0) {
          x0 = DX[0][c2]; x1 = DX[1][c2]; y0 = DY[0][c2]; y1 = DY[1][c2];
        } else {
          x0 = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, DX[0][c2 + 1]), __builtin_bit_cast(uint32_t, DX[0][c2]), 0x05040302u));
          x1 = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, DX[1][c2 + 1]), __builtin_bit_cast(uint32_t, DX[1][c2]), 0x05040302u));
          y0 = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, DY[0][c2 + 1]), __builtin_bit_cast(uint32_t, DY[0][c2]), 0x05040302u));
          y1 = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm(__builtin_bit_cast(uint32_t, DY[1][c2 + 1]), __builtin_bit_cast(uint32_t, DY[1][c2]), 0x05040302u));
        }
        int ax = lk_dot2_bias(x0, wT, 1 << (W_BITS - 1)), ay = lk_dot2_bias(y0, wT, 1 << (W_BITS - 1));
        int ai = lk_dot2_bias(__builtin_bit_cast(lk_s2, LK_PAIR(d[1], c + 1)), wT, 1 << (W_BITS - 5 - 1));
        ax = __builtin_amdgcn_sdot2(x1, wB, ax, false);
        ay = __builtin_amdgcn_sdot2(y1, wB, ay, false);
        ai = __builtin_amdgcn_sdot2(__builtin_bit_cast(lk_s2, LK_PAIR(d[2], c + 1)), wB, ai, false);
        const bool on = c0 + c < LK_WIN;  // window column 31 of the second half does not exist
        ix[hh] = on ? (ax >> W_BITS) : 0;
        iy[hh] = on ? (ay >> W_BITS) : 0;
        iv[hh] = on ? (ai >> (W_BITS - 5)) : 0;
      }
      tI[c2] = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm((uint32_t)iv[1], (uint32_t)iv[0], 0x05040100u));
      tX[c2] = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm((uint32_t)ix[1], (uint32_t)ix[0], 0x05040100u));
      tY[c2] = __builtin_bit_cast(lk_s2, __builtin_amdgcn_perm((uint32_t)iy[1], (uint32_t)iy[0], 0x05040100u));
      a11 = __builtin_amdgcn_sdot2(tX[c2], tX[c2], a11, false);
      a12 = __builtin_amdgcn_sdot2(tX[c2], tY[c2], a12, false);
      a22 = __builtin_amdgcn_sdot2(tY[c2], tY[c2], a22, false);
    }
  } else {
#pragma unroll
    for (int c = 0; c < 8; c++) {
      tI[c] = lk_s2{0, 0};
      tX[c] = lk_s2{0, 0};
      tY[c] = lk_s2{0, 0};
    }
  }
}

// One level's template from the image: stage the source patch (rows ipy-1 .. ipy+32, columns ipx-1 .. ipx+34), Scharr + bilinear
// interpolation, the three Hessian sums over the wave.  Returns whether the staging took the index-reflecting path.
__device__ __forceinline__ bool lk_template_level(const uint8_t* img, int W, int H, int pitch, int bx, int by, int ipx, int ipy, int iw00,
                                                  int iw01, int iw10, int iw11, uint8_t* patch, int lane, lk_s2 (&tI)[8], lk_s2 (&tX)[8],
                                                  lk_s2 (&tY)[8], long long& iA11, long long& iA12, long long& iA22) {
  __syncthreads();
  const bool slow = lk_load_patch(img, W, H, pitch, bx, by, ipx - 1, ipy - 1, LK_PROWS, patch);
  __syncthreads();
  int a11 = 0, a12 = 0, a22 = 0;
  // every pixel the Scharr stencil is evaluated at lies inside the image -> no border masks (wave-uniform test)
  const bool interior = ipx >= 0 && ipx + 32 <= W - 1 && ipy >= 0 && ipy + 31 <= H - 1;
  const lk_s2 wT = lk_s2{(short)iw00, (short)iw01}, wB = lk_s2{(short)iw10, (short)iw11};
  if (interior)
    lk_template<true>(patch, lane, ipx, ipy, W, H, wT, wB, tI, tX, tY, a11, a12, a22);
  else
    lk_template<false>(patch, lane, ipx, ipy, W, H, wT, wB, tI, tX, tY, a11, a12, a22);
  lk_wave_sum3_wide(a11, a12, a22, iA11, iA12, iA22);
  return slow;
}
// The same as a CALL, for the temporal launch: there nearly every template comes from the cache, and with the computation out of line
// (its own register allocation, results handed over through the caller's stack) the kernel's hot path -- cache loads, region staging,
// iterations -- fits a register budget that lets twice as many waves share a SIMD.
struct LKTmpl {
  uint32_t w[24];
  long long a11, a12, a22;
};
__device__ __noinline__ void lk_template_level_cold(const uint8_t* img, int W, int H, int pitch, int bx, int by, int ipx, int ipy, int iw00,
                                                    int iw01, int iw10, int iw11, uint8_t* patch, int lane, LKTmpl* out) {
  lk_s2 tI[8], tX[8], tY[8];
  long long a11, a12, a22;
  lk_template_level(img, W, H, pitch, bx, by, ipx, ipy, iw00, iw01, iw10, iw11, patch, lane, tI, tX, tY, a11, a12, a22);
#pragma unroll
  for (int k = 0; k < 8; k++) {
    out->w[k] = __builtin_bit_cast(uint32_t, tI[k]);
    out->w[8 + k] = __builtin_bit_cast(uint32_t, tX[k]);
    out->w[16 + k] = __builtin_bit_cast(uint32_t, tY[k]);
  }
  out->a11 = a11;
  out->a12 = a12;
  out->a22 = a22;
}

// one level's templates into a cache slot: the 24 template registers of the 64 lanes as six 1 KB rows; lane 63 (window row 31: no template)
// carries the level's six floats (LK_TC_HDR's comment) in the place of its first six tI registers
__device__ __forceinline__ void lk_tc_store_level(uint32_t* tc_ptr, int level, int lane, const lk_s2 (&tI)[8], const lk_s2 (&tX)[8],
                                                  const lk_s2 (&tY)[8], float A11, float A12, float A22, float D, float minEig, float invD) {
  lk_u4* dst = reinterpret_cast<lk_u4*>(tc_ptr + LK_TC_HDR + (size_t)level * LK_TC_LVL) + lane;
  uint32_t wI[8];
#pragma unroll
  for (int k = 0; k < 8; k++) wI[k] = __builtin_bit_cast(uint32_t, tI[k]);
  if (lane == 63) {
    wI[0] = __float_as_uint(A11); wI[1] = __float_as_uint(A12); wI[2] = __float_as_uint(A22);
    wI[3] = __float_as_uint(D); wI[4] = __float_as_uint(minEig); wI[5] = __float_as_uint(invD);
  }
#pragma unroll
  for (int k = 0; k < 2; k++) {
    __builtin_nontemporal_store(lk_u4{wI[4 * k], wI[4 * k + 1], wI[4 * k + 2], wI[4 * k + 3]}, dst + 64 * k);
    __builtin_nontemporal_store(lk_u4{__builtin_bit_cast(uint32_t, tX[4 * k]), __builtin_bit_cast(uint32_t, tX[4 * k + 1]),
                                      __builtin_bit_cast(uint32_t, tX[4 * k + 2]), __builtin_bit_cast(uint32_t, tX[4 * k + 3])}, dst + 64 * (2 + k));
    __builtin_nontemporal_store(lk_u4{__builtin_bit_cast(uint32_t, tY[4 * k]), __builtin_bit_cast(uint32_t, tY[4 * k + 1]),
                                      __builtin_bit_cast(uint32_t, tY[4 * k + 2]), __builtin_bit_cast(uint32_t, tY[4 * k + 3])}, dst + 64 * (4 + k));
  }
}

// What the kernels read of a pyramid: ONE 64-byte descriptor per level, made from the caller's PyrSel by launch_lk_track.  PyrSel is
// structure-of-arrays, and with the level a run-time index every field of it cost a scalar load with its own address arithmetic and wait
// (~18 per level and wave, profiles/r32_lk_level_setup.md); a descriptor is one s_load_dwordx16.  The slot choice is resolved as far as the
// host can: b[k] is the base a wave whose stream's slot is k reads (ImgSel::flip applied; both the same where the level has no slot array).
struct alignas(64) LKLevel {
  const uint8_t* b[2];
  const uint8_t* const* ind;  // ImgSel::ind
  size_t stride;              // bytes between consecutive streams
  int w, h, pitch, bx, by;
  int pad_[3];
};
static_assert(sizeof(LKLevel) == 64, "one s_load_dwordx16");
struct alignas(64) LKPyr {
  LKLevel lvl[LK_MAX_LEVELS];
  const int* cur;  // the slot array of the lowest level that has one (all levels share it: fill_pyr), or nullptr
  int levels;
};
static LKPyr lk_pyr(const PyrSel& P) {
  LKPyr q{};
  q.levels = P.levels;
  for (int l = P.levels < LK_MAX_LEVELS ? P.levels : LK_MAX_LEVELS - 1; l >= 0; l--) {
    const ImgSel& I = P.lvl[l];
    LKLevel& V = q.lvl[l];
    V.b[0] = I.b[I.cur ? (I.flip & 1) : 0];
    V.b[1] = I.b[I.cur ? ((I.flip & 1) ^ 1) : 0];
    V.ind = I.ind;
    V.stride = P.stride[l];
    V.w = P.w[l], V.h = P.h[l], V.pitch = P.pitch[l], V.bx = P.bx[l], V.by = P.by[l];
    if (I.cur) q.cur = I.cur;
  }
  return q;
}

// Base address of one pyramid level for stream s.  The slot choice cur[s] (a global load the compiler may not hoist: memory could have
// changed) is read ONCE per wave and passed in: every level of a pyramid that selects by slot shares one slot array (fill_pyr); ind0 =
// the already loaded base of an indirect level 0.  A level then costs kernel-argument reads only, no dependent global round trip.
__device__ __forceinline__ const uint8_t* lk_level_ptr(const LKLevel& V, int level, int s, int kc, const uint8_t* ind0) {
  if (V.ind) return (level == 0 ? ind0 : *V.ind) + (size_t)s * V.stride;
  return (kc ? V.b[1] : V.b[0]) + (size_t)s * V.stride;
}

#ifndef FLVIS_LK_WAVES
#define FLVIS_LK_WAVES 4  // (build-variant knob: waves per SIMD the register allocation aims at)
#endif
#ifndef FLVIS_LK_WAVES_T
#define FLVIS_LK_WAVES_T 4  // ... of the temporal launch (its template computation is out of line)
#endif
// 4 waves per SIMD (<= 128 VGPRs): this kernel is latency-bound (PMC: VALU busy ~20%), occupancy is what pays
// ROLE names the launch in the profiles and fixes what the template cache may do: 0 the stand-alone entry point (no cache), 1 the
// tracker's temporal launch (may take templates from the cache), 2 its stereo launch (may store them).  (A stereo launch fed by
// a kernel that made the tracked landmarks' templates ahead was not faster: profiles/r06_templates_ahead.md.)
#ifdef FLVIS_LK_UTIL
// (build variant, scripts/lk_util.py: how full the chip is during an LK launch.  Every wave that tracks a point leaves its start and end
// time (wall clock, 100 MHz) in a slot of its own: [launch kind: role % 3][the launch's slot, 8 of them][wave][start, end])
__device__ unsigned long long g_lk_wt[3][8][32768][2];
#define LK_UTIL_BEGIN const unsigned long long lk_t0_ = wall_clock64(); const unsigned lk_widx_ = (blockIdx.y * gridDim.x + blockIdx.x) & 32767u;
#define LK_UTIL_END(ROLE)                                                              \
  if (threadIdx.x == 0) {                                                              \
    unsigned long long* u_ = g_lk_wt[(ROLE) % 3][prm.dbg_slot & 7][lk_widx_];          \
    u_[0] = lk_t0_;                                                                    \
    u_[1] = wall_clock64();                                                            \
  }
#else
#define LK_UTIL_BEGIN
#define LK_UTIL_END(ROLE)
#endif
template <int ROLE>
__device__ __forceinline__ void lk_track_body(const LKPyr& prev, const LKPyr& next, const float* __restrict__ prev_pts,
                                              float* __restrict__ next_pts, uint8_t* __restrict__ status,
                                              const int* __restrict__ count, int nmax, const LKParams& prm,
                                              const int* __restrict__ active) {
  // XCD-aware workgroup -> (stream, point) map: workgroup b is observed to run on XCD b % 8 (each XCD has its own 4 MiB
  // L2), so a stream's workgroups are renumbered onto one XCD and its two pyramids (~0.8 MB) are fetched from HBM once
  // instead of once per XCD.  A bijection whenever the grid size is a multiple of 8; speed only, never correctness.
  int s = blockIdx.y, bx = blockIdx.x;
  {
    const int G = gridDim.x, N = G * gridDim.y;
    if ((N & 7) == 0) {
      const int L = bx + G * s;
      const int Lp = (L & 7) * (N >> 3) + (L >> 3);
      s = Lp / G;
      bx = Lp - s * G;
    }
  }
  if (active && !active[s]) return;
  int n = count[s];
  if (n > nmax) n = nmax;
  if (bx >= n) return;
  LK_UTIL_BEGIN
  __shared__ __attribute__((aligned(16))) uint8_t patch[LK_RROWS * LK_RS + 12];  // template patch, then search region
  const int lane = threadIdx.x;
  const int kc_prev = prev.cur ? prev.cur[s] : 0, kc_next = next.cur ? next.cur[s] : 0;
  const uint8_t* const ind_prev0 = prev.lvl[0].ind ? *prev.lvl[0].ind : nullptr;
  const uint8_t* const ind_next0 = next.lvl[0].ind ? *next.lvl[0].ind : nullptr;
  const int r = lane >> 1;
  const int c0 = (lane & 1) * 16;
  const int W_BITS = 14;
  // (epsilon^2 in a VECTOR register pair: the scalar registers are oversubscribed by the two pyramids' argument blocks, and the compiler
  // re-read this kernel argument with an s_load + s_waitcnt in front of the convergence test of EVERY iteration)
  double eps2 = prm.eps2;
  if (ROLE == 1) asm volatile("" : "+v"(eps2));  // (the launches with registers to spare: 121 of 128; the others are at 128)
  const float FLT_SCALE = 1.f / (1 << 20);
  const float halfWin = (LK_WIN - 1) * 0.5f;

  for (int pb = bx; pb < n; pb += gridDim.x) {
    // (order of dispatch: a launch ends one wave's duration after its last workgroup has started, so the long points should start first.
    //  prm.order 1: the stream's points from the last to the first -- a frame's new landmarks, which the stereo matcher has no depth to
    //  start from, are appended behind the tracked ones)
    const int p = prm.order == 1 ? n - 1 - pb : pb;
    const size_t pi = ((size_t)s * nmax + p) * 2;
    // (one address for the whole wave, but a per-lane load: without the read-first-lane the compiler takes the positions, and with them
    // every test of the level and of the iteration, for divergent, and guards each with an exec-mask save and restore)
    const float ppx0 = lk_uniform(prev_pts[pi]), ppy0 = lk_uniform(prev_pts[pi + 1]);
    float nx = lk_uniform(next_pts[pi]), ny = lk_uniform(next_pts[pi + 1]);
    int st = 1;
    // template cache: the slot this point stores its templates in (stereo matcher), or the slot it may take them from (temporal
    // tracker: valid if it was written for this very position of this very image)
    uint32_t* tc_ptr = nullptr;
    bool tc_store = false, tc_hit = false;
    uint32_t tc_mask = 0;
    if (ROLE == 2 && prm.tc_mode == 1) {
      if (p < prm.tc_cap) {
        tc_store = true;
        tc_ptr = prm.tc + ((size_t)s * prm.tc_cap + p) * prm.tc_stride;
      }
    } else if (ROLE == 1 && prm.tc_mode == 2) {
      // the caller has compared the slot's header (position bits, tag) with this point: code = slot | (mask of stored levels << 16), or -1
      const int code = __builtin_amdgcn_readfirstlane(prm.tc_slot[(size_t)s * nmax + p]);
      if (code >= 0 && (code & 0xffff) < prm.tc_cap) {
        tc_ptr = prm.tc + ((size_t)s * prm.tc_cap + (code & 0xffff)) * prm.tc_stride;
        tc_hit = true;
        tc_mask = (uint32_t)code >> 16;
      }
    }
    lk_u4 pq[6] = {};  // templates of level pq_level, in flight or arrived (-1: none)
    int pq_level = -1;
    for (int level = prev.levels; level >= 0; level--) {
      // 2^-level from its bits: the float that (float)(1. / (1 << level)) is, without the double-precision division (14 vector
      // instructions per level)
      static_assert(LK_MAX_LEVELS <= 126, "2^-level is a normal float");
      const float sc = __uint_as_float((uint32_t)(127 - level) << 23);
      // the level's two descriptors: everything a wave needs of the level, one wide scalar load per pyramid
      const LKLevel PV = prev.lvl[level], NV = next.lvl[level];
      float ppx = ppx0 * sc, ppy = ppy0 * sc;
      float npx, npy;
      if (level == prev.levels) {
        if (prm.use_initial) {
          npx = nx * sc;
          npy = ny * sc;
        } else {
          npx = ppx;
          npy = ppy;
        }
      } else {
        npx = nx * 2.f;
        npy = ny * 2.f;
      }
      nx = npx;
      ny = npy;
      const int W = PV.w, H = PV.h;
      ppx -= halfWin;
      ppy -= halfWin;
      const int ipx = (int)floorf(ppx), ipy = (int)floorf(ppy);
      if (ipx < -LK_WIN || ipx >= W || ipy < -LK_WIN || ipy >= H) {
        if (level == 0) st = 0;
        continue;
      }
      float a = ppx - (float)ipx, b = ppy - (float)ipy;
      int iw00 = __float2int_rn((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
      int iw01 = __float2int_rn(a * (1.f - b) * (float)(1 << W_BITS));
      int iw10 = __float2int_rn((1.f - a) * b * (float)(1 << W_BITS));
      int iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;

      // ---- template.  Either from the cache (the stereo matcher of the previous frame made this very template: same image, same
      // position), or computed: stage source patch rows ipy-1..ipy+32, cols ipx-1..ipx+34, Scharr + bilinear interpolation
      lk_s2 tI[8], tX[8], tY[8];  // pixel pairs (c, c+1)
      long long iA11 = 0, iA12 = 0, iA22 = 0;
      // A = the Hessian sums as floats, D its determinant (1 / D from the iterations on), minEig the smaller eigenvalue per pixel: from
      // the sums, or -- a cached level -- as the stereo launch computed them from the same sums (cD: its 1 / D)
      float A11 = 0.f, A12 = 0.f, A22 = 0.f, D = 0.f, minEig = 0.f, cD = 0.f;
      const bool cached = ROLE == 1 && tc_hit && ((tc_mask >> level) & 1u);
      // (the launches that may take templates from the cache look at the search image before the template stage: see below)
      constexpr bool kEarlyRegion = ROLE == 1;
      int JW = 0, JH = 0;
      const uint8_t* Jimg = nullptr;
      if (kEarlyRegion) {
        JW = NV.w, JH = NV.h;
        Jimg = lk_level_ptr(NV, level, s, kc_next, ind_next0);
      }
      bool region_ok = false;
      int RX0 = 0, RY0 = 0;
      if (cached) {
        if (prm.stats_tc && lane == 0) atomicAdd(&prm.stats_tc[0], 1ull);
        if (pq_level != level) {  // (the top level, or the level above did not get this far)
          const lk_u4* src = reinterpret_cast<const lk_u4*>(tc_ptr + LK_TC_HDR + (size_t)level * LK_TC_LVL) + lane;
#pragma unroll
          for (int k = 0; k < 6; k++) pq[k] = __builtin_nontemporal_load(src + 64 * k);
        }
        if (kEarlyRegion) {
        // the search region of the level's FIRST iteration, staged while the templates travel: its position is the level's start position,
        // known before the templates are (a cached level needs no source patch, so the LDS buffer is free) -- one memory round trip per
        // level instead of two.  Same region, same bytes as the iteration would stage itself.
        {
          const int einx = (int)floorf(npx - halfWin), einy = (int)floorf(npy - halfWin);
          if (!(einx < -LK_WIN || einx >= JW || einy < -LK_WIN || einy >= JH)) {
            RX0 = (einx - LK_RM) & ~3;
            RY0 = einy - LK_RM;
            __syncthreads();
            const bool slow = lk_load_region(Jimg, JW, JH, NV.pitch, NV.bx, NV.by, RX0, RY0, patch);
            __syncthreads();
            if (prm.stats_tc && slow && lane == 0) atomicAdd(&prm.stats_tc[2], 1ull);
            region_ok = true;
          }
        }
        }
        lk_u4 q[6];
#pragma unroll
        for (int k = 0; k < 6; k++) q[k] = pq[k];
        pq_level = -1;
        // (the level's floats ride in lane 63's registers: the lanes of window row 31 hold no template)
        A11 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)q[0].x, 63));
        A12 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)q[0].y, 63));
        A22 = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)q[0].z, 63));
        D = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)q[0].w, 63));
        minEig = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)q[1].x, 63));
        cD = __uint_as_float((uint32_t)__builtin_amdgcn_readlane((int)q[1].y, 63));
#pragma unroll
        for (int k = 0; k < 2; k++) {
          tI[4 * k + 0] = lk_as_s2(q[k].x); tI[4 * k + 1] = lk_as_s2(q[k].y);
          tI[4 * k + 2] = lk_as_s2(q[k].z); tI[4 * k + 3] = lk_as_s2(q[k].w);
          tX[4 * k + 0] = lk_as_s2(q[2 + k].x); tX[4 * k + 1] = lk_as_s2(q[2 + k].y);
          tX[4 * k + 2] = lk_as_s2(q[2 + k].z); tX[4 * k + 3] = lk_as_s2(q[2 + k].w);
          tY[4 * k + 0] = lk_as_s2(q[4 + k].x); tY[4 * k + 1] = lk_as_s2(q[4 + k].y);
          tY[4 * k + 2] = lk_as_s2(q[4 + k].z); tY[4 * k + 3] = lk_as_s2(q[4 + k].w);
        }
      } else if (ROLE == 1) {
        LKTmpl T;
        lk_template_level_cold(lk_level_ptr(PV, level, s, kc_prev, ind_prev0), W, H, PV.pitch, PV.bx, PV.by, ipx, ipy, iw00,
                               iw01, iw10, iw11, patch, lane, &T);
#pragma unroll
        for (int k = 0; k < 8; k++) {
          tI[k] = lk_as_s2(T.w[k]);
          tX[k] = lk_as_s2(T.w[8 + k]);
          tY[k] = lk_as_s2(T.w[16 + k]);
        }
        // (read back from the stack, per lane: said to be uniform, or the update they scale, and so every test of the iteration loop of
        // this launch, counts as divergent -- also for the levels whose floats come out of the cache by read-lane)
        iA11 = lk_uniform64(T.a11);
        iA12 = lk_uniform64(T.a12);
        iA22 = lk_uniform64(T.a22);
      } else {
        const bool slow = lk_template_level(lk_level_ptr(PV, level, s, kc_prev, ind_prev0), W, H, PV.pitch, PV.bx, PV.by, ipx,
                                            ipy, iw00, iw01, iw10, iw11, patch, lane, tI, tX, tY, iA11, iA12, iA22);
        if (prm.stats_tc && slow && lane == 0) atomicAdd(&prm.stats_tc[1], 1ull);
      }
      float invD = 0.f;
      if (!cached) {
        A11 = (float)iA11 * FLT_SCALE, A12 = (float)iA12 * FLT_SCALE, A22 = (float)iA22 * FLT_SCALE;
        D = A11 * A22 - A12 * A12;
        minEig = __fdiv_rn(A22 + A11 - sqrtf((A11 - A22) * (A11 - A22) + 4.f * A12 * A12), (float)(2 * LK_WIN * LK_WIN));
      }
      const bool skip = minEig < prm.min_eig || D < 1.1920929e-07f;
      if (cached) {
        invD = cD;
      } else if (!skip) {
        invD = __fdiv_rn(1.f, D);
      }
      if (ROLE == 2 && tc_store) {
        lk_tc_store_level(tc_ptr, level, lane, tI, tX, tY, A11, A12, A22, D, minEig, invD);
        tc_mask |= 1u << level;
      }
      if (skip) {
        if (level == 0) st = 0;
        continue;
      }
      D = invD;
      npx -= halfWin;
      npy -= halfWin;
      float pdx = 0.f, pdy = 0.f;
      if (!kEarlyRegion) {
        JW = NV.w, JH = NV.h;
        Jimg = lk_level_ptr(NV, level, s, kc_next, ind_next0);
      }
      int iters_run = 0;
      for (int j = 0; j < prm.max_iter; j++) {
        iters_run = j + 1;
        const int inx = (int)floorf(npx), iny = (int)floorf(npy);
        // (inx < -LK_WIN || inx >= JW as ONE unsigned comparison: inx + LK_WIN wraps to a huge value exactly when it is negative, and
        // a conversion that saturated at either end of int lands outside as well)
        if ((unsigned)inx + (unsigned)LK_WIN >= (unsigned)(JW + LK_WIN) || (unsigned)iny + (unsigned)LK_WIN >= (unsigned)(JH + LK_WIN)) {
          if (level == 0) st = 0;
          break;
        }
        a = npx - (float)inx;
        b = npy - (float)iny;
        iw00 = __float2int_rn((1.f - a) * (1.f - b) * (float)(1 << W_BITS));
        iw01 = __float2int_rn(a * (1.f - b) * (float)(1 << W_BITS));
        iw10 = __float2int_rn((1.f - a) * b * (float)(1 << W_BITS));
        iw11 = (1 << W_BITS) - iw00 - iw01 - iw10;
        // (inx, iny and the region's corner are within a window of the image here: the differences cannot wrap)
        if (!region_ok || (unsigned)(inx - RX0) > 15u || (unsigned)(iny - RY0) > (unsigned)(2 * LK_RM)) {
          RX0 = (inx - LK_RM) & ~3;
          RY0 = iny - LK_RM;
          __syncthreads();
          const bool slow = lk_load_region(Jimg, JW, JH, NV.pitch, NV.bx, NV.by, RX0, RY0, patch);
          __syncthreads();
          if (prm.stats_tc && slow && lane == 0) atomicAdd(&prm.stats_tc[2], 1ull);
          region_ok = true;
        }
        int b1, b2;
        {
          // (all 64 lanes, no exec mask: the lanes of window row 31 read rows iny - RY0 + 31 and + 32 <= 40 of the 41 staged ones and
          // the same columns as every other lane, and add nothing -- their tX and tY are 0, computed here or taken from the cache, where
          // lane 63's tI carries the level's floats)
          const int bx = inx - RX0 + c0, sh = bx & 3;
          const uint8_t* rp = patch + (iny - RY0 + r) * LK_RS + (bx & ~3);
          uint32_t e[2][5];
#pragma unroll
          for (int q = 0; q < 2; q++) {
            uint32_t dd[6];
#pragma unroll
            for (int k = 0; k < 6; k++) dd[k] = *reinterpret_cast<const uint32_t*>(rp + q * LK_RS + 4 * k);
#pragma unroll
            for (int k = 0; k < 5; k++) e[q][k] = __builtin_amdgcn_alignbyte(dd[k + 1], dd[k], sh);
          }
          const lk_s2 wT = lk_s2{(short)iw00, (short)iw01}, wB = lk_s2{(short)iw10, (short)iw11};
          // The two pixels of a pair side by side: the second dot product of a pixel stands behind the other pixel's first.  (Pipelining
          // the pairs against each other as well -- pair c's interpolation issued before pair c - 1's residual, behind scheduling fences --
          // took the last ten wait-state no-ops out of this loop and measured no gain: profiles/r31_lk_diet.md.)
          // 0 < acc < 2^22: pixels <= 255, the four weights sum to 2^14, three of them are >= 0 and the fourth, 2^14 minus the three
          // rounded ones, is >= -1 (each rounding adds at most 1/2, and where the exact fourth weight is 0 one of the others is exact), so
          // acc >= 256 - 255 and acc <= 255 * (2^14 + 1) + 256
          b1 = 0, b2 = 0;
#pragma unroll
          for (int c2 = 0; c2 < 8; c2++) {
            const int c = 2 * c2;
            int acc0 = lk_dot2_bias(__builtin_bit_cast(lk_s2, LK_PAIR(e[0], c)), wT, 1 << (W_BITS - 5 - 1));
            int acc1 = lk_dot2_bias(__builtin_bit_cast(lk_s2, LK_PAIR(e[0], c + 1)), wT, 1 << (W_BITS - 5 - 1));
            acc0 = __builtin_amdgcn_sdot2(__builtin_bit_cast(lk_s2, LK_PAIR(e[1], c)), wB, acc0, false);
            acc1 = __builtin_amdgcn_sdot2(__builtin_bit_cast(lk_s2, LK_PAIR(e[1], c + 1)), wB, acc1, false);
            const lk_s2 diff = lk_pack_shr<W_BITS - 5>(acc0, acc1) - tI[c2];
            // columns >= 31 have tX = tY = 0, so they add nothing
            b1 = __builtin_amdgcn_sdot2(diff, tX[c2], b1, false);
            b2 = __builtin_amdgcn_sdot2(diff, tY[c2], b2, false);
          }
        }
        float sb1, sb2;
        lk_wave_sum2_f32(b1, b2, sb1, sb2);
        const float fb1 = sb1 * FLT_SCALE, fb2 = sb2 * FLT_SCALE;
        const float ddx = (A12 * fb2 - A22 * fb1) * D;
        const float ddy = (A12 * fb1 - A11 * fb2) * D;
        npx += ddx;
        npy += ddy;
        nx = npx + halfWin;
        ny = npy + halfWin;
        // (eps2 sits in vector registers, which makes the comparison divergent to the compiler: the ballot says it is one decision)
        if (__builtin_amdgcn_ballot_w64((double)ddx * (double)ddx + (double)ddy * (double)ddy <= eps2) != 0) break;
        if (j > 0 && fabs((double)(ddx + pdx)) < 0.01 && fabs((double)(ddy + pdy)) < 0.01) {
          nx -= ddx * 0.5f;
          ny -= ddy * 0.5f;
          break;
        }
        pdx = ddx;
        pdy = ddy;
      }
      if (prm.stats && lane == 0) {
        atomicAdd(&prm.stats[2 * level], (unsigned long long)iters_run);
        atomicAdd(&prm.stats[2 * level + 1], 1ull);
      }
      if (st && level == 0) {  // error stage of calcOpticalFlowPyrLK: final window must still start inside
        const float fx = nx - halfWin, fy = ny - halfWin;
        const int inx = (int)floorf(fx), iny = (int)floorf(fy);
        if (inx < -LK_WIN || inx >= JW || iny < -LK_WIN || iny >= JH) st = 0;
      }
    }
    if (lane == 0) {
      next_pts[pi] = nx;
      next_pts[pi + 1] = ny;
      status[(size_t)s * nmax + p] = (uint8_t)st;
      if (ROLE == 2 && tc_store) {
        tc_ptr[0] = __float_as_uint(ppx0);
        tc_ptr[1] = __float_as_uint(ppy0);
        *reinterpret_cast<long long*>(tc_ptr + 2) = prm.tc_tag[s];
        tc_ptr[4] = tc_mask;
      }
    }
  }
  LK_UTIL_END(ROLE)
}

// the three launches (named apart in the profiles; the register budget is per launch kind)
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FLVIS_LK_WAVES, FLVIS_LK_WAVES))) void k_lk_track(
    LKPyr prev, LKPyr next, const float* __restrict__ prev_pts, float* __restrict__ next_pts, uint8_t* __restrict__ status,
    const int* __restrict__ count, int nmax, LKParams prm, const int* __restrict__ active) {
  lk_track_body<0>(prev, next, prev_pts, next_pts, status, count, nmax, prm, active);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FLVIS_LK_WAVES_T, FLVIS_LK_WAVES_T))) void k_lk_track_temporal(
    LKPyr prev, LKPyr next, const float* __restrict__ prev_pts, float* __restrict__ next_pts, uint8_t* __restrict__ status,
    const int* __restrict__ count, int nmax, LKParams prm, const int* __restrict__ active) {
  lk_track_body<1>(prev, next, prev_pts, next_pts, status, count, nmax, prm, active);
}
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(FLVIS_LK_WAVES, FLVIS_LK_WAVES))) void k_lk_track_stereo(
    LKPyr prev, LKPyr next, const float* __restrict__ prev_pts, float* __restrict__ next_pts, uint8_t* __restrict__ status,
    const int* __restrict__ count, int nmax, LKParams prm, const int* __restrict__ active) {
  lk_track_body<2>(prev, next, prev_pts, next_pts, status, count, nmax, prm, active);
}

int lk_tc_slot_dwords(int levels) { return LK_TC_HDR + (levels + 1) * LK_TC_LVL; }

void launch_lk_track(hipStream_t st, const PyrSel& prev_sel, const PyrSel& next_sel, const float* prev_pts, float* next_pts,
                     uint8_t* status, const int* count, int nmax, int S, LKParams prm, const int* active, int max_pts, int role) {
  // one wave per point; the kernel strides by the grid width, so any width is correct.  Sized by the caller's bound on
  // the point count (the tracker holds <= 16 regions x max_region_feature_num landmarks), rounded so that the XCD-aware
  // renumbering stays a bijection (grid size a multiple of 8)
  int gx = nmax < 512 ? nmax : 512;
  if (max_pts > 0 && max_pts < gx) gx = (max_pts + 7) & ~7;
  if (gx > nmax) gx = nmax;
  const LKPyr prev = lk_pyr(prev_sel), next = lk_pyr(next_sel);
  if (role == 1)
    hipLaunchKernelGGL(k_lk_track_temporal, dim3(gx, S), dim3(64), 0, st, prev, next, prev_pts, next_pts, status, count, nmax, prm, active);
  else if (role == 2)
    hipLaunchKernelGGL(k_lk_track_stereo, dim3(gx, S), dim3(64), 0, st, prev, next, prev_pts, next_pts, status, count, nmax, prm, active);
  else
    hipLaunchKernelGGL(k_lk_track, dim3(gx, S), dim3(64), 0, st, prev, next, prev_pts, next_pts, status, count, nmax, prm, active);
}

}  // namespace flvis

#ifdef FLVIS_LK_UTIL
extern "C" int flvis_debug_lk_util(unsigned long long* out, int reset) {  // out: 3 * 8 * 32768 * 2 values
  const size_t bytes = sizeof(unsigned long long) * 3 * 8 * 32768 * 2;
  if (out && hipMemcpyFromSymbol(out, HIP_SYMBOL(flvis::g_lk_wt), bytes) != hipSuccess) return -1;
  if (reset) {
    void* dp = nullptr;
    if (hipGetSymbolAddress(&dp, HIP_SYMBOL(flvis::g_lk_wt)) != hipSuccess || hipMemset(dp, 0, bytes) != hipSuccess) return -1;
  }
  return 0;
}
#endif
