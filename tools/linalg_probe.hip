// tools/linalg_probe.hip -- runs ONE of the small dense solvers of lsqrrecipes_amd/csrc/{small_linalg,wave_linalg}.h on a
// batch of matrices, in one launch, so that tests/test_gpu_small_linalg.py can compare the device's results with the host
// build of the same headers (tests/host_math/driver.cpp) and with exact solutions (tests/linalg_families.py).
//   hipcc --offload-arch=gfx950 -O3 -std=c++20 -ffp-contract=off -o tools/linalg_probe tools/linalg_probe.hip
//   tools/linalg_probe INPUT OUTPUT
// INPUT:  one or more sections: 8 doubles {routine, count, m, n, variant, tol, 0, 0}, then count problems of in_stride
//         doubles each.  One launch per section.
// OUTPUT: per section 2 doubles {count, out_stride}, then count results of out_stride doubles each.
// Matrices are row-major in both files.  Exit status 0 only when every HIP call succeeded.
//
// routine (in_stride -> out_stride), one THREAD per problem (small_linalg.h):
//   1 sym_eig         a[n*n]               -> w[n], v[n*n]
//   2 svd_jacobi      a[m*n]               -> u[m*n], s[n], v[n*n]
//   3 pinv_solve      a[m*n], b[m]         -> rank, x[n]                 (tol: absolute threshold)
//   4 spd_solve_chol  g[n*n], rhs[n]       -> accepted, x[n]             (tol: the value x is filled with beforehand)
//   5 spd_solve_eig   g[n*n], rhs[n]       -> rank, x[n]                 (tol: rtol)
//   6 lsqr_sincos     x                    -> sin, cos
// one WORKGROUP (or wave) per problem, the system staged column-major in LDS with lda = n | 1 as k_estimate_dense and
// k_estimate_dense_w4 stage it (wave_linalg.h); m == n:
//   10 elimination    a[n*n], b[n]         -> accepted, x[n]     variant 0 block_gepp_solve<256>, 1 wave_gepp_solve (four
//                                                                systems per workgroup), 2 wave_gepp_solve_reg64 (n = 64)
//   11 pinv           a[n*n], b[n]         -> rank, x[n], v[n*n] variant 0 block_pinv_solve<256>, 1 <64>, 2 <64, 12, 12> and
//                                                                3 <64, 9, 9> with LDA 13 (the US kernels'); tol absolute
//   12 jacobi         a[n*n], b[n]         -> sweeps, us[n*n], v[n*n]   the sweeps alone, variants as for 11
//      11 and 12 also: variant 4 <64, 31, 31> and 5 <256, 31, 31> with LDA 31 (the plane phantom's sizes), 6 and 7 the
//      generic code with 128 and 512 threads, which split a column pair over as many lanes (4, 16) as those two do
//   13 null vector    a[n*n], b[n]         -> n_positive, x[n]   variant 0 block_null_vector<256>, 1 <64>, 2 <64, 31, 31> and
//                                                                3 <256, 31, 31> with LDA 31 (the plane phantom's)
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../lsqrrecipes_amd/csrc/small_linalg.h"
#include "../lsqrrecipes_amd/csrc/wave_linalg.h"

using namespace lsqr;

#define CK(x)                                                                  \
  do {                                                                         \
    hipError_t e_ = (x);                                                       \
    if (e_ != hipSuccess) {                                                    \
      fprintf(stderr, "%s:%d %s\n", __FILE__, __LINE__, hipGetErrorString(e_)); \
      exit(1);                                                                 \
    }                                                                          \
  } while (0)

enum { R_SYM_EIG = 1, R_SVD = 2, R_PINV = 3, R_CHOL = 4, R_SPD_EIG = 5, R_SINCOS = 6, R_GEPP = 10, R_WPINV = 11,
       R_JACOBI = 12, R_NULLVEC = 13 };

// one thread per problem: lane 0 of a wave of its own, so that problems of different lengths do not wait for each other
// (lsqr_sincos: every lane, one argument each)
__global__ __launch_bounds__(64) void k_thread(int routine, int count, int m, int n, double tol, double *in,
                                               size_t in_stride, double *out, size_t out_stride, double *work,
                                               size_t work_stride) {
  if (routine == R_SINCOS) {
    const size_t i = (size_t)blockIdx.x * 64 + threadIdx.x;
    if (i < (size_t)count) lsqr_sincos(in[i], out + 2 * i, out + 2 * i + 1);
    return;
  }
  const int h = blockIdx.x;
  if (threadIdx.x != 0 || h >= count) return;
  double *p = in + (size_t)h * in_stride, *o = out + (size_t)h * out_stride, *w = work + (size_t)h * work_stride;
  switch (routine) {
    case R_SYM_EIG: sym_eig(n, p, o, o + n); break;
    case R_SVD:
      svd_jacobi(m, n, p, n, o + m * n, o + m * n + n);
      for (int i = 0; i < m * n; i++) o[i] = p[i];
      break;
    case R_PINV: o[0] = pinv_solve(m, n, p, n, p + m * n, tol, o + 1, w, w + n); break;
    case R_CHOL:
      for (int i = 0; i < n; i++) o[1 + i] = tol;
      o[0] = spd_solve_chol(n, p, p + n * n, o + 1, w) ? 1.0 : 0.0;
      break;
    case R_SPD_EIG: o[0] = spd_solve_eig(n, p, p + n * n, tol, o + 1, w); break;
    default: break;
  }
}

__global__ __launch_bounds__(256) void k_gepp_block(int n, const double *in, size_t in_stride, double *out,
                                                    size_t out_stride) {
  extern __shared__ double sm[];
  const int lda = n | 1, tid = threadIdx.x;
  double *A = sm, *b = A + n * lda, *x = b + n;
  const double *p = in + (size_t)blockIdx.x * in_stride;
  double *o = out + (size_t)blockIdx.x * out_stride;
  for (int idx = tid; idx < n * n; idx += 256) A[(idx % n) * lda + idx / n] = p[idx];
  for (int l = tid; l < n; l += 256) b[l] = p[n * n + l];
  __syncthreads();
  const bool ok = block_gepp_solve<256>(n, A, lda, b, x);
  __syncthreads();
  if (tid == 0) o[0] = ok ? 1.0 : 0.0;
  for (int j = tid; j < n; j += 256) o[1 + j] = ok ? x[j] : __builtin_nan("");
}

__global__ __launch_bounds__(256) void k_gepp_wave(int count, int n, const double *in, size_t in_stride, double *out,
                                                   size_t out_stride) {
  extern __shared__ double sm[];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int h = blockIdx.x * 4 + wave;
  if (h >= count) return;  // wave-uniform; no workgroup barrier below
  const int lda = n | 1;
  double *A = sm + (size_t)wave * (n * lda + 2 * n), *b = A + n * lda, *x = b + n;
  const double *p = in + (size_t)h * in_stride;
  double *o = out + (size_t)h * out_stride;
  for (int l = 0; l < n; l++) {  // lane = column, as k_estimate_dense_w4 reads a row
    if (lane < n) A[lane * lda + l] = p[l * n + lane];
    if (lane == 0) b[l] = p[n * n + l];
  }
  __builtin_amdgcn_wave_barrier();
  const bool ok = wave_gepp_solve(n, A, lda, b, x);
  __builtin_amdgcn_wave_barrier();
  if (lane == 0) o[0] = ok ? 1.0 : 0.0;
  if (lane < n) o[1 + lane] = ok ? x[lane] : __builtin_nan("");
}

__global__ __launch_bounds__(64) void k_gepp_reg64(const double *in, size_t in_stride, double *out, size_t out_stride) {
  const int lane = threadIdx.x;
  const double *p = in + (size_t)blockIdx.x * in_stride;
  double *o = out + (size_t)blockIdx.x * out_stride;
  double a[64], xv;
#pragma unroll
  for (int c = 0; c < 64; c++) a[c] = p[lane * 64 + c];
  const bool ok = wave_gepp_solve_reg64(a, p[64 * 64 + lane], xv);
  if (lane == 0) o[0] = ok ? 1.0 : 0.0;
  o[1 + lane] = ok ? xv : __builtin_nan("");
}

// routines 11, 12, 13; M = N = 0: the generic code, lda = n | 1; else compile-time sizes with leading dimension LDA
template <int T, int M, int N, int LDA>
__global__ __launch_bounds__(T) void k_jacobi(int routine, int n, double tol, const double *in, size_t in_stride,
                                              double *out, size_t out_stride) {
  extern __shared__ double sm[];
  __shared__ int s_int;
  const int lda = M > 0 ? LDA : (n | 1), tid = threadIdx.x;
  double *A = sm, *V = A + n * lda, *b = V + n * lda, *cw = b + n, *x = cw + n;
  const double *p = in + (size_t)blockIdx.x * in_stride;
  double *o = out + (size_t)blockIdx.x * out_stride;
  for (int idx = tid; idx < n * n; idx += T) A[(idx % n) * lda + idx / n] = p[idx];
  for (int l = tid; l < n; l += T) b[l] = p[n * n + l];
  __syncthreads();
  if (routine == R_WPINV) {
    const int rank = block_pinv_solve<T, M, N>(n, n, A, lda, V, lda, b, tol, 0.0, x, cw);
    if (tid == 0) o[0] = rank;
    for (int j = tid; j < n; j += T) o[1 + j] = x[j];
    for (int idx = tid; idx < n * n; idx += T) o[1 + n + idx] = V[(idx % n) * lda + idx / n];
  } else if (routine == R_JACOBI) {
    block_jacobi_prescale<T>(n, n, A, lda);
    int sweeps;
    if constexpr (M > 0) sweeps = block_jacobi_svd_fixed<T, M, N>(A, lda, V, lda);
    else sweeps = block_jacobi_svd<T>(n, n, A, lda, V, lda);
    __syncthreads();
    if (tid == 0) o[0] = sweeps;
    for (int idx = tid; idx < n * n; idx += T) {
      o[1 + idx] = A[(idx % n) * lda + idx / n];
      o[1 + n * n + idx] = V[(idx % n) * lda + idx / n];
    }
  } else {
    block_null_vector<T, M, N>(n, n, A, lda, V, lda, x, &s_int);
    __syncthreads();
    if (tid == 0) o[0] = s_int;
    for (int j = tid; j < n; j += T) o[1 + j] = x[j];
  }
}

template <int T, int M, int N, int LDA>
static void launch_jacobi(int routine, int count, int n, double tol, const double *in, size_t in_stride, double *out,
                          size_t out_stride) {
  if (M > 0 && n != N) {
    fprintf(stderr, "variant needs n = %d\n", N);
    exit(2);
  }
  const int lda = M > 0 ? LDA : (n | 1);
  const size_t lds = sizeof(double) * ((size_t)2 * n * lda + 3 * n);
  CK(hipFuncSetAttribute((const void *)k_jacobi<T, M, N, LDA>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL((k_jacobi<T, M, N, LDA>), dim3(count), dim3(T), lds, 0, routine, n, tol, in, in_stride, out,
                     out_stride);
}

// one section: 0 done, > 0 an error
static int run_section(const double *hdr, FILE *f, FILE *fo) {
  const int routine = (int)hdr[0], count = (int)hdr[1], m = (int)hdr[2], n = (int)hdr[3], variant = (int)hdr[4];
  const double tol = hdr[5];
  const bool wave_routine = routine >= R_GEPP;
  if (count < 1 || count > (1 << 22) || n < 1 || n > 64 || m < n || m > 128 || (wave_routine && m != n) ||
      (routine != R_SINCOS && count > 4096)) {
    fprintf(stderr, "bad header: routine %d count %d m %d n %d\n", routine, count, m, n);
    return 2;
  }
  size_t in_stride = 0, out_stride = 0, work_stride = 0;
  switch (routine) {
    case R_SYM_EIG: in_stride = (size_t)n * n, out_stride = n + (size_t)n * n; break;
    case R_SVD: in_stride = (size_t)m * n, out_stride = (size_t)m * n + n + (size_t)n * n; break;
    case R_PINV: in_stride = (size_t)m * n + m, out_stride = 1 + n, work_stride = n + (size_t)n * n; break;
    case R_CHOL: in_stride = (size_t)n * n + n, out_stride = 1 + n, work_stride = (size_t)n * n + n; break;
    case R_SPD_EIG: in_stride = (size_t)n * n + n, out_stride = 1 + n, work_stride = (size_t)2 * n * n + 3 * n; break;
    case R_SINCOS: in_stride = 1, out_stride = 2; break;
    case R_GEPP: in_stride = (size_t)n * n + n, out_stride = 1 + n; break;
    case R_WPINV: in_stride = (size_t)n * n + n, out_stride = 1 + n + (size_t)n * n; break;
    case R_JACOBI: in_stride = (size_t)n * n + n, out_stride = 1 + (size_t)2 * n * n; break;
    case R_NULLVEC: in_stride = (size_t)n * n + n, out_stride = 1 + n; break;
    default: fprintf(stderr, "unknown routine %d\n", routine); return 2;
  }
  std::vector<double> in((size_t)count * in_stride), out((size_t)count * out_stride);
  if (fread(in.data(), sizeof(double), in.size(), f) != in.size()) {
    fprintf(stderr, "the input is shorter than its header says\n");
    return 2;
  }
  double *d_in, *d_out, *d_work = nullptr;
  CK(hipMalloc(&d_in, in.size() * sizeof(double)));
  CK(hipMalloc(&d_out, out.size() * sizeof(double)));
  if (work_stride) CK(hipMalloc(&d_work, (size_t)count * work_stride * sizeof(double)));
  CK(hipMemcpy(d_in, in.data(), in.size() * sizeof(double), hipMemcpyHostToDevice));
  CK(hipMemset(d_out, 0, out.size() * sizeof(double)));
  if (!wave_routine) {
    const unsigned blocks = routine == R_SINCOS ? (unsigned)((count + 63) / 64) : (unsigned)count;
    hipLaunchKernelGGL(k_thread, dim3(blocks), dim3(64), 0, 0, routine, count, m, n, tol, d_in, in_stride, d_out,
                       out_stride, d_work, work_stride);
  } else if (routine == R_GEPP) {
    const int lda = n | 1;
    if (variant == 0) {
      const size_t lds = sizeof(double) * ((size_t)n * lda + 2 * n);
      CK(hipFuncSetAttribute((const void *)k_gepp_block, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(k_gepp_block, dim3(count), dim3(256), lds, 0, n, d_in, in_stride, d_out, out_stride);
    } else if (variant == 1) {
      const size_t lds = sizeof(double) * 4 * ((size_t)n * lda + 2 * n);
      CK(hipFuncSetAttribute((const void *)k_gepp_wave, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
      hipLaunchKernelGGL(k_gepp_wave, dim3((count + 3) / 4), dim3(256), lds, 0, count, n, d_in, in_stride, d_out,
                         out_stride);
    } else if (variant == 2 && n == 64) {
      hipLaunchKernelGGL(k_gepp_reg64, dim3(count), dim3(64), 0, 0, d_in, in_stride, d_out, out_stride);
    } else {
      fprintf(stderr, "elimination: variant %d at n = %d\n", variant, n);
      return 2;
    }
  } else {
    const bool nullvec = routine == R_NULLVEC;
    if (variant == 0) launch_jacobi<256, 0, 0, 0>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 1) launch_jacobi<64, 0, 0, 0>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 2 && !nullvec) launch_jacobi<64, 12, 12, 13>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 3 && !nullvec) launch_jacobi<64, 9, 9, 13>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 2) launch_jacobi<64, 31, 31, 31>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 3) launch_jacobi<256, 31, 31, 31>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 4) launch_jacobi<64, 31, 31, 31>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 5) launch_jacobi<256, 31, 31, 31>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 6) launch_jacobi<128, 0, 0, 0>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else if (variant == 7) launch_jacobi<512, 0, 0, 0>(routine, count, n, tol, d_in, in_stride, d_out, out_stride);
    else {
      fprintf(stderr, "unknown variant %d\n", variant);
      return 2;
    }
  }
  CK(hipGetLastError());
  CK(hipDeviceSynchronize());
  CK(hipMemcpy(out.data(), d_out, out.size() * sizeof(double), hipMemcpyDeviceToHost));
  CK(hipFree(d_in));
  CK(hipFree(d_out));
  if (d_work) CK(hipFree(d_work));
  const double ohdr[2] = {(double)count, (double)out_stride};
  if (fwrite(ohdr, sizeof(double), 2, fo) != 2 || fwrite(out.data(), sizeof(double), out.size(), fo) != out.size()) {
    fprintf(stderr, "cannot write the output\n");
    return 1;
  }
  return 0;
}

int main(int argc, char **argv) {
  if (argc != 3) {
    fprintf(stderr, "usage: linalg_probe INPUT OUTPUT\n");
    return 2;
  }
  FILE *f = fopen(argv[1], "rb"), *fo = fopen(argv[2], "wb");
  if (!f || !fo) {
    fprintf(stderr, "cannot open %s or %s\n", argv[1], argv[2]);
    return 2;
  }
  double hdr[8];
  int sections = 0;
  for (;;) {
    const size_t got = fread(hdr, sizeof(double), 8, f);
    if (got == 0) break;
    if (got != 8) {
      fprintf(stderr, "truncated section header in %s\n", argv[1]);
      return 2;
    }
    const int rc = run_section(hdr, f, fo);
    if (rc) return rc;
    sections++;
  }
  if (fclose(fo) != 0 || !sections) {
    fprintf(stderr, "nothing written to %s\n", argv[2]);
    return 1;
  }
  return 0;
}
