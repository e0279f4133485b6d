// Microbenchmark: v_mfma_f32_4x4x1_16b_f32 (16 independent 4x4 blocks, K = 1, fp32 in / fp32 accumulate) against
// v_mfma_f32_16x16x4_f32, the form the exact blend backward used before.
//   hipcc --offload-arch=gfx950 -O3 scripts/mb_mfma_4x4.hip -o build/mb_mfma_4x4 && ./build/mb_mfma_4x4
// 1. Layout (exact integer data, asymmetric A and B): lane l = 4 b + t supplies A[b][row t] and B[b][column t]; result
//    register r of lane 4 b + t holds D[b][row r][column t].  Also the two permlane swaps the kernel sums rows with:
//    permlane32_swap(x, y) -> (x of lanes 0..31 | y of lanes 0..31, x of lanes 32..63 | y of lanes 32..63), and
//    permlane16_swap(x, y) -> the same per 32-lane half with 16-lane rows.
// 2. Cycles per instruction (s_memtime, one wave per SIMD) with 1, 2 and 3 independent accumulator chains: 1 chain gives
//    the dependent-accumulator latency, enough chains the issue interval.
// 3. Overlap with VALU of OTHER waves (as scripts/mb_mfma_valu.hip): 8 waves per SIMD, all FMA / all MFMA / half and half.
#include <hip/hip_runtime.h>
#include <cstdio>
typedef float f32x4 __attribute__((ext_vector_type(4)));

__global__ void layout_kernel(const float *a, const float *b, float *d, unsigned *sw) {
  const int l = threadIdx.x;
  const f32x4 z = {0.0f, 0.0f, 0.0f, 0.0f};
  const f32x4 r = __builtin_amdgcn_mfma_f32_4x4x1f32(a[l], b[l], z, 0, 0, 0);
  for (int i = 0; i < 4; i++) d[i * 64 + l] = r[i];
  const auto s32 = __builtin_amdgcn_permlane32_swap((unsigned)l, 100u + l, false, false);
  const auto s16 = __builtin_amdgcn_permlane16_swap((unsigned)l, 100u + l, false, false);
  sw[l] = s32[0]; sw[64 + l] = s32[1]; sw[128 + l] = s16[0]; sw[192 + l] = s16[1];
}

template <int kForm, int kChains>   // kForm 0: 4x4x1_16b, 1: 16x16x4
__global__ void latency_kernel(float *out, long long *cyc, int iters) {
  f32x4 acc[3] = {};
  const float x = 1.0f + threadIdx.x * 1e-6f, y = 0.999f;
  const long long t0 = clock64();
  for (int i = 0; i < iters; i++) {
#pragma unroll
    for (int u = 0; u < 8; u++)
#pragma unroll
      for (int c = 0; c < kChains; c++)
        acc[c] = kForm == 0 ? __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, acc[c], 0, 0, 0)
                            : __builtin_amdgcn_mfma_f32_16x16x4f32(x, y, acc[c], 0, 0, 0);
  }
  const long long t1 = clock64();
  float r = 0.0f;
  for (int c = 0; c < kChains; c++) r += acc[c][0] + acc[c][3];
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
  if (threadIdx.x == 0 && blockIdx.x == 0) cyc[0] = t1 - t0;
}

template <int MODE>   // 0: all FMA, 1: all MFMA 4x4x1, 2: even waves FMA + odd waves MFMA
__global__ void overlap_kernel(float *out, int iters) {
  const int wave = threadIdx.x >> 6;
  const bool do_mfma = MODE == 1 || (MODE == 2 && (wave & 1));
  float r = 0.0f;
  if (do_mfma) {
    f32x4 a0 = {0, 0, 0, 0}, a1 = a0, a2 = a0, a3 = a0;
    const float x = threadIdx.x * 1e-3f, y = 1.0001f;
    for (int i = 0; i < 4 * iters; i++) {   // 16 MFMAs of 8 cycles = 128 cycles, as 32 FMAs
      a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a2, 0, 0, 0); a3 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a3, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a2, 0, 0, 0); a3 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a3, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a2, 0, 0, 0); a3 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a3, 0, 0, 0);
      a0 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a0, 0, 0, 0); a1 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a1, 0, 0, 0);
      a2 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a2, 0, 0, 0); a3 = __builtin_amdgcn_mfma_f32_4x4x1f32(x, y, a3, 0, 0, 0);
    }
    r = a0.x + a1.y + a2.z + a3.w;
  } else {
    float x0 = threadIdx.x, x1 = x0 + 1, x2 = x0 + 2, x3 = x0 + 3, x4 = x0 + 4, x5 = x0 + 5, x6 = x0 + 6, x7 = x0 + 7;
    const float a = 1.0001f, b = 0.5f;
    for (int i = 0; i < 4 * iters; i++) {
      asm volatile("v_fma_f32 %0, %0, %8, %9\n v_fma_f32 %1, %1, %8, %9\n v_fma_f32 %2, %2, %8, %9\n v_fma_f32 %3, %3, %8, %9\n"
                   "v_fma_f32 %4, %4, %8, %9\n v_fma_f32 %5, %5, %8, %9\n v_fma_f32 %6, %6, %8, %9\n v_fma_f32 %7, %7, %8, %9\n"
                   : "+v"(x0), "+v"(x1), "+v"(x2), "+v"(x3), "+v"(x4), "+v"(x5), "+v"(x6), "+v"(x7) : "v"(a), "v"(b));
    }
    r = x0 + x1 + x2 + x3 + x4 + x5 + x6 + x7;
  }
  out[blockIdx.x * blockDim.x + threadIdx.x] = r;
}

template <int kForm, int kChains>
double cycles_per_mfma(float *d, long long *cyc) {
  const int iters = 2000;
  latency_kernel<kForm, kChains><<<256, 256>>>(d, cyc, iters);   // one wave per SIMD
  latency_kernel<kForm, kChains><<<256, 256>>>(d, cyc, iters);
  long long c = 0;
  (void)hipMemcpy(&c, cyc, sizeof(c), hipMemcpyDeviceToHost);
  return (double)c / (iters * 8.0 * kChains);
}

template <int MODE>
float overlap_ms(float *d, int iters) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0); (void)hipEventCreate(&e1);
  overlap_kernel<MODE><<<256 * 4, 512>>>(d, iters);   // 8 waves per SIMD
  (void)hipEventRecord(e0);
  overlap_kernel<MODE><<<256 * 4, 512>>>(d, iters);
  (void)hipEventRecord(e1); (void)hipEventSynchronize(e1);
  float ms; (void)hipEventElapsedTime(&ms, e0, e1);
  return ms;
}

int main() {
  // 1. layout
  float ha[64], hb[64], hd[256];
  unsigned hs[256];
  for (int l = 0; l < 64; l++) { ha[l] = (float)(l % 7 + 1 + 8 * (l / 4)); hb[l] = (float)(3 * (l % 4) + 1 + 16 * (l / 4)); }
  float *da, *db, *dd; unsigned *ds;
  (void)hipMalloc(&da, sizeof ha); (void)hipMalloc(&db, sizeof hb); (void)hipMalloc(&dd, sizeof hd); (void)hipMalloc(&ds, sizeof hs);
  (void)hipMemcpy(da, ha, sizeof ha, hipMemcpyHostToDevice); (void)hipMemcpy(db, hb, sizeof hb, hipMemcpyHostToDevice);
  layout_kernel<<<1, 64>>>(da, db, dd, ds);
  (void)hipMemcpy(hd, dd, sizeof hd, hipMemcpyDeviceToHost); (void)hipMemcpy(hs, ds, sizeof hs, hipMemcpyDeviceToHost);
  int bad = 0;
  for (int l = 0; l < 64; l++)
    for (int r = 0; r < 4; r++) {
      const int blk = l / 4, t = l % 4;
      if (hd[r * 64 + l] != ha[4 * blk + r] * hb[4 * blk + t]) bad++;
    }
  int bad_sw = 0;
  for (int l = 0; l < 64; l++) {
    const unsigned x32 = l < 32 ? l : 100u + (l - 32), y32 = l < 32 ? l + 32u : 100u + l;
    const int row = l >> 4, base = l & ~31, in = l & 15;
    const unsigned x16 = (row & 1) ? 100u + (base + in) : (unsigned)l, y16 = (row & 1) ? 100u + l : (unsigned)(base + 16 + in);
    bad_sw += (hs[l] != x32) + (hs[64 + l] != y32) + (hs[128 + l] != x16) + (hs[192 + l] != y16);
  }
  printf("layout 4x4x1_16b: %s (%d of 256 outputs differ from D[b][r][t] = A[4b+r] B[4b+t] at reg r, lane 4b+t)\n",
         bad ? "MISMATCH" : "ok", bad);
  printf("permlane swaps: %s (%d mismatches)\n", bad_sw ? "MISMATCH" : "ok", bad_sw);
  // 2. cycles
  float *d; long long *cyc;
  (void)hipMalloc(&d, 256 * 4 * 512 * 4); (void)hipMalloc(&cyc, sizeof(long long));
  printf("cycles per MFMA, one wave per SIMD (1 / 2 / 3 independent accumulators):\n");
  printf("  4x4x1_16b_f32 : %.1f / %.1f / %.1f\n", cycles_per_mfma<0, 1>(d, cyc), cycles_per_mfma<0, 2>(d, cyc), cycles_per_mfma<0, 3>(d, cyc));
  printf("  16x16x4_f32   : %.1f / %.1f / %.1f\n", cycles_per_mfma<1, 1>(d, cyc), cycles_per_mfma<1, 2>(d, cyc), cycles_per_mfma<1, 3>(d, cyc));
  // 3. overlap
  const int iters = 4000;
  const float t0 = overlap_ms<0>(d, iters), t1 = overlap_ms<1>(d, iters), t2 = overlap_ms<2>(d, iters);
  printf("4x4x1 vs VALU of other waves: all FMA %.3f ms, all MFMA %.3f ms, mixed %.3f ms; overlap would give %.3f, no overlap %.3f\n",
         t0, t1, t2, (t0 > t1 ? t0 : t1) / 2, (t0 + t1) / 2);
  return bad || bad_sw ? 1 : 0;
}
