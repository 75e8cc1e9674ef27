// assign_rigid.h -- lsqr_assign_rigid / lsqr_refine_rigid: lsqr_assign / lsqr_refine (assign.h) for the closed-form
// models whose parameters hold no point: absolute orientation (ls_type 0, or 2: weighted pairs), pivot calibration and
// ray intersection (rigid.h).  Every record of the context's upload goes to the NEAREST of up to 64 models it agrees
// with, and (refine) every model is fitted again on its own records, round after round, on the device.  The rounds
// are assign.h's loop, assign_rounds, with the family AssignRigid<M> of this file; the decision for one record is
// assign_one<M>, which the pass and lsqr_assign_rigid_host both run.
//
//   k_assign_rigid_pass    chunk blockIdx.x of the upload: assign_pass_chunk (assign.h) with kAssignRigidPerLane<M>
//                          records per lane and, for absolute orientation, the origins of the table
//   k_assign_rigid_first   absolute orientation, once per refine call: first[m] = the lowest index of a record that is
//                          finite and agrees with row m as passed in.  A workgroup takes a chunk as the pass does, the
//                          lane's records in registers, row by row at wave-uniform addresses; the lane's lowest index,
//                          a min over the wave, a 32-bit atomicMin in LDS per wave that has one, then ONE 64-bit
//                          integer atomicMin per (workgroup, model present) on the 64 words of `first`: a min of
//                          integers, so the order of the workgroups does not matter
//   k_assign_rigid_origin  first[m] -> org[m][0..6) = (first, second) of that record; zeros for a model without one
//   k_assign_rigid_solve   one workgroup per model: assign_sum_chunks, then assign_refit about the model's origin
//                          (k_assign_solve's shape)
//
// The origin of model m's moment block (fit_origin_offset is -1 here: the parameters hold no point):
//   ray       the model's own point, row slots 0..2, as for the plane: it moves with the row from round to round
//   pivot     none: PivotModel::accumulate and ::solve read no origin
//   absolute orientation   (first, second) of record first[m], fixed for the whole call.  This is lsqr_ls_fit's rule
//             for a mask without a winner ("the first record whose mask bit is set") applied to the mask of row m at
//             entry, so the origin is finite and lies among the model's data even when record 0 is an outlier or NaN.
//             A model no record agrees with at entry can never get one -- rows change only by a refit, and a refit
//             needs records --, so its origin (zeros) is never read.
//
// Order of the sums: kAssignRigidChunk<M> -- 2048 records for absolute orientation and the ray, 1024 for the pivot --
// fixes it, as kAssignChunk does for assign.h: within a chunk the lane's records in index order, the __shfl_down tree,
// the four waves in order; then the chunks in order.  A model absent from a chunk adds +0.0.  Model m's block, and so
// its iterates, are a function of its own records, their positions in the upload, its own row and its own origin: not
// of the grid, of the other rows of the call or of where m sits among them.  Nothing is summed with a floating-point
// atomic, so two runs of one call give the same bits.
//
// Budget (launch bounds kBlock = 4 waves; DESIGN.md section 14.6 has the table): kAssignPerLane = 8 records of the
// pivot's 12-slot frame are 96 doubles a lane, so the pivot keeps 4 (48 doubles, as the ray's 8 x 6) and absolute
// orientation 8 x 7; beside them one moment block (16 / 22 / 10 doubles), the labels and the residuals.  No kernel of
// this file uses scratch.  LDS of the pass as in assign.h (under 2 KiB here); of the solve one tile of 256 chunks'
// blocks, the moment block and the workspace (21 .. 47 KiB).
#pragma once
#include "assign.h"
#include "rigid.h"

namespace lsqr {

// records a lane keeps in registers, and so the records per workgroup (fixes the moment sums' order)
template <class M> constexpr int kAssignRigidPerLane = 8;
template <> constexpr int kAssignRigidPerLane<PivotModel> = 4;
template <class M> constexpr uint32_t kAssignRigidChunk = (uint32_t)kAssignRigidPerLane<M> * kBlock;
// the origins come from a table made at entry (else from the model's row, or there is none)
template <class M> constexpr bool kAssignRigidTable = false;
template <> constexpr bool kAssignRigidTable<AbsOrModel> = true;

// The model k_assign_rigid_solve hands to assign_refit, and the doubles of its workspace.  The pivot's 6 x 6 solve
// indexes its matrices in loops, so as locals they live in scratch: PivotSolveWs is PivotModel whose solve takes them
// from the kernel's LDS workspace (solve_small's solve_ws hook).  The normal equations are assembled as
// PivotModel::solve assembles them, entry for entry, and solved by the same spd_solve_eig call: the same bits.
// (PivotModel::solve itself is left as it is, so the kernels that run it -- k_solve, k_many_solve -- do not change.)
struct PivotSolveWs : PivotModel {
  static LSQR_HD bool solve_ws(const double *m, const double *, const ModelConsts &, double *par, double *ws) {
    const double n = m[0];
    if (n < 3.0) return false;
    double *G = ws, *rhs = ws + 36, *work = ws + 42;  // 36, 6 and 2 * 36 + 18 doubles
    int q = 1;
    for (int a = 0; a < 3; a++)
      for (int b = a; b < 3; b++, q++) G[a * 6 + b] = G[b * 6 + a] = m[q];
    for (int k = 0; k < 3; k++)
      for (int a = 0; a < 3; a++) {
        G[(3 + k) * 6 + a] = -m[7 + 3 * k + a];
        G[a * 6 + 3 + k] = -m[7 + 3 * k + a];
      }
    for (int a = 0; a < 3; a++)
      for (int b = 0; b < 3; b++) G[(3 + a) * 6 + 3 + b] = (a == b) ? n : 0.0;
    for (int a = 0; a < 3; a++) {
      rhs[a] = -m[16 + a];
      rhs[3 + a] = m[19 + a];
    }
    return spd_solve_eig(6, G, rhs, 1e-13, par, work) == 6;
  }
};
template <> constexpr int kAssignOrigin<PivotSolveWs> = 0;
template <class M> struct AssignRigidSolve { typedef M type; static constexpr int WS = 8; };
template <> struct AssignRigidSolve<PivotModel> {
  typedef PivotSolveWs type;
  static constexpr int WS = 42 + 2 * 36 + 18;
};

#if defined(__HIPCC__)
// chunk blockIdx.x of the context's n records; the arguments of k_assign_moments (assign.h).  org_tab: the origins
// [model][kAssignOrigin<M>] (read only where kAssignRigidTable<M>)
template <class M, bool WITH_MOMENTS>
__global__ __launch_bounds__(kBlock) void k_assign_rigid_pass(
    const double *__restrict__ data, size_t stride, uint32_t n, const double *__restrict__ rows, int n_models,
    const double *__restrict__ org_tab, ModelConsts mc, int32_t *__restrict__ labels, double *__restrict__ residuals,
    const int32_t *__restrict__ old, unsigned long long *__restrict__ counters, double *__restrict__ partials) {
  constexpr uint32_t CH = kAssignRigidChunk<M>;
  const uint32_t c0 = blockIdx.x * CH, left = n - c0;  // (c0 < n: no wrap)
  if constexpr (WITH_MOMENTS) partials += (size_t)blockIdx.x * n_models * AccLs<M>::N;
  assign_pass_chunk<M, WITH_MOMENTS, kAssignRigidPerLane<M>>(
      data + (size_t)c0 * stride, stride, left < CH ? left : CH, rows, n_models, 0, mc, labels + c0,
      residuals ? residuals + c0 : nullptr, old ? old + c0 : nullptr, counters + ASG_CHANGED, counters + ASG_COUNT,
      partials, nullptr, kAssignRigidTable<M> ? org_tab : nullptr);
}

// first[m], m < n_models (set to ~0 by the caller): the lowest i < n whose record is finite -- every loaded slot, the
// weight included -- and agrees with rows[m]
template <class M>
__global__ __launch_bounds__(kBlock) void k_assign_rigid_first(const double *__restrict__ data, size_t stride,
                                                               uint32_t n, const double *__restrict__ rows,
                                                               int n_models, ModelConsts mc,
                                                               unsigned long long *__restrict__ first) {
  constexpr int R = kAssignRigidPerLane<M>;
  constexpr uint32_t CH = kAssignRigidChunk<M>;
  __shared__ uint32_t s_first[kAssignMaxModels];
  const uint32_t c0 = blockIdx.x * CH, left = n - c0, cnt = left < CH ? left : CH;
  const double qnan = __builtin_nan("");
  if (threadIdx.x < kAssignMaxModels) s_first[threadIdx.x] = ~0u;
  double x[R][M::REC];
#pragma unroll
  for (int j = 0; j < R; j++) {
    const uint32_t i = (uint32_t)j * kBlock + threadIdx.x;
    const bool in = i < cnt;
    M::load(data + (size_t)(c0 + (in ? i : 0)) * stride, mc, x[j]);
    if (!in || !assign_finite<M>(x[j])) {
#pragma unroll
      for (int d = 0; d < (int)M::REC; d++) x[j][d] = qnan;  // NaN agrees with nothing
    }
  }
  __syncthreads();
  for (int m = 0; m < n_models; m++) {
    const double *row = rows + (size_t)m * M::SP;  // wave-uniform: scalar loads
    uint32_t mine = ~0u;
#pragma unroll
    for (int j = R - 1; j >= 0; j--)  // downwards: the lowest index is written last
      if (M::agree(row, x[j], mc)) mine = (uint32_t)j * kBlock + threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) {
      const uint32_t v = __shfl_xor(mine, o);
      mine = v < mine ? v : mine;
    }
    if ((threadIdx.x & 63) == 0 && mine != ~0u) atomicMin(&s_first[m], mine);
  }
  __syncthreads();
  if ((int)threadIdx.x < n_models && s_first[threadIdx.x] != ~0u)
    atomicMin(&first[threadIdx.x], (unsigned long long)c0 + s_first[threadIdx.x]);
}

// org[m][k], k < NO: slot k of record first[m]; zeros where first[m] is ~0
__global__ __launch_bounds__(kBlock) void k_assign_rigid_origin(const unsigned long long *__restrict__ first,
                                                                const double *__restrict__ data, size_t stride,
                                                                int n_models, int NO, double *__restrict__ org) {
  for (int e = threadIdx.x; e < n_models * NO; e += kBlock) {
    const unsigned long long i = first[e / NO];
    org[e] = i == ~0ull ? 0.0 : data[(size_t)i * stride + (e % NO)];
  }
}

// one workgroup per model m: k_assign_solve (assign.h) about the model's origin -- org_tab[m] where
// kAssignRigidTable<M>, else row m's slots 0 .. kAssignOrigin<M>
template <class M>
__global__ __launch_bounds__(kBlock) void k_assign_rigid_solve(const double *__restrict__ partials, uint32_t chunks,
                                                               int n_models, const double *__restrict__ org_tab,
                                                               ModelConsts mc, double *rows,
                                                               unsigned long long *counters) {
  constexpr int N = M::NMOM;
  constexpr int kTile = 256;  // chunks per tile: 20 KiB of LDS at N = 10, 44 KiB at N = 22
  __shared__ double s_t[kTile * N];
  __shared__ double mom[MOM_MAX];
  __shared__ double ws[AssignRigidSolve<M>::WS];
  __shared__ SolveOut so;
  const int m = blockIdx.x;
  assign_sum_chunks<N, kTile>(partials + (size_t)m * N, (size_t)n_models * N, chunks, s_t, mom);
  if (threadIdx.x != 0) return;
  const unsigned long long cnt = counters[ASG_COUNT + m];
  counters[ASG_USED + m] = cnt;
  const double *org_m = kAssignRigidTable<M> ? org_tab + (size_t)m * kAssignOrigin<M> : nullptr;
  typedef typename AssignRigidSolve<M>::type S;
  counters[ASG_OK + m] = assign_refit<S>(mom, rows + (size_t)m * M::SP, cnt, 0, mc, ws, &so, org_m) ? 1 : 0;
}

// The rigid models' family of the round loop (assign.h: assign_rounds): AssignClosed<M> -- its buffers, its pinned
// layout, its way of turning parameters into scan rows and back -- with the chunk size, the pass and the solve of this
// file, and for absolute orientation the origin pre-pass, enqueued once behind the rows of a refine call.
template <class M>
struct AssignRigid : AssignClosed<M> {
  using AssignClosed<M>::B;
  static_assert((int)M::NMOM <= 64 && (int)M::NMOM <= (int)MOM_MAX, "one lane per moment");

  static uint32_t chunks_of(uint32_t n) {
    return (uint32_t)(((uint64_t)n + kAssignRigidChunk<M> - 1) / kAssignRigidChunk<M>);
  }
  int reserve(AssignJob &J, bool refine) {
    MANYCHK(many_grow(B.d_par, (size_t)kAssignMaxModels * 16));
    if (refine) {
      MANYCHK(many_grow(B.core.d_partials, (size_t)chunks_of(J.n) * J.n_models * M::NMOM));
      if constexpr (kAssignRigidTable<M>) {
        MANYCHK(many_grow(B.d_org, (size_t)kAssignMaxModels * kAssignOrigin<M>));
        MANYCHK(many_grow(B.d_first, (size_t)kAssignMaxModels));
      }
    }
    return LSQR_OK;
  }
  int rows_up(AssignJob &J, double *h_rows) {
    const int st = AssignClosed<M>::rows_up(J, h_rows);
    if (st != LSQR_OK) return st;
    if constexpr (kAssignRigidTable<M>) {
      if (J.max_rounds > 0) {  // the origins, from the rows as passed in
        const int nm = (int)J.n_models;
        MANYCHK(hipMemsetAsync(B.d_first, 0xFF, sizeof(unsigned long long) * kAssignMaxModels, J.stream));
        hipLaunchKernelGGL((k_assign_rigid_first<M>), dim3(chunks_of(J.n)), dim3(kBlock), 0, J.stream, J.data, J.stride,
                           J.n, B.core.d_rows, nm, J.mc, B.d_first);
        MANYCHK(hipGetLastError());
        hipLaunchKernelGGL(k_assign_rigid_origin, dim3(1), dim3(kBlock), 0, J.stream, B.d_first, J.data, J.stride, nm,
                           (int)kAssignOrigin<M>, B.d_org);
        MANYCHK(hipGetLastError());
      }
    }
    return LSQR_OK;
  }
  int pass(AssignJob &J, bool last, int32_t *lab, double *res, const int32_t *old) {
    const int nm = (int)J.n_models;
    const uint32_t chunks = chunks_of(J.n);
    AssignCore &C = B.core;
    if (last)
      hipLaunchKernelGGL((k_assign_rigid_pass<M, false>), dim3(chunks), dim3(kBlock), 0, J.stream, J.data, J.stride,
                         J.n, C.d_rows, nm, nullptr, J.mc, lab, res, old, C.d_cnt, nullptr);
    else
      hipLaunchKernelGGL((k_assign_rigid_pass<M, true>), dim3(chunks), dim3(kBlock), 0, J.stream, J.data, J.stride,
                         J.n, C.d_rows, nm, B.d_org, J.mc, lab, res, old, C.d_cnt, C.d_partials);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
  int refit(AssignJob &J, const int32_t *) {
    const int nm = (int)J.n_models;
    hipLaunchKernelGGL((k_assign_rigid_solve<M>), dim3(nm), dim3(kBlock), 0, J.stream, B.core.d_partials,
                       chunks_of(J.n), nm, B.d_org, J.mc, B.core.d_rows, B.core.d_cnt);
    MANYCHK(hipGetLastError());
    return LSQR_OK;
  }
};
#endif  // __HIPCC__

}  // namespace lsqr
