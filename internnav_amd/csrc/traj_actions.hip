// The step's action table from the sampled System-1 trajectories, on the device (gfx950): what vln_utils.traj_to_actions (vln_utils.py:63-136)
// computes on the host per env - un-normalise, cumulative sum, mean over the S samples, greedy pure-pursuit discretisation - for B envs in one launch.
//
// One workgroup of ONE wave per env; every rounding of the host function is reproduced in its order:
//   1. x, y of traj [B, S, T, 3] (f32 | bf16) times 0.25 in the input's precision (exact: a power of two), then per (sample, coordinate) a SEQUENTIAL
//      fp32 running sum over t that starts from the first element - np.cumsum on the float32 array. A lane owns one (sample, coordinate) chain of a
//      group of 32 samples and leaves its sums of a chunk of 32 steps in LDS.
//   2. the lanes change roles and own one (t, coordinate) column of the chunk: the column's fp64 accumulator (LDS) takes the widened sums of the
//      group's samples in sample order, the first sample by copy - np.mean(axis=0) = add.reduce over the outer axis, then ONE IEEE division by S.
//      A column is summed by one lane, so no cross-lane reduction order enters. Row 0 of the mean trajectory is the leading zero row.
//   3. the pure-pursuit loop runs in fp64, redundantly and uniformly on all 64 lanes; only the nearest-point search is spread over the lanes
//      (np.argmin: first minimum, lowest index wins ties - a butterfly over (distance, index) pairs). Python's % (result takes the divisor's
//      sign) and round-half-to-even (rint) are restated; x*x + y*y is two roundings as in numpy: contraction is OFF in this file.
//      atan2 / cos / sin differ from the host's libm by a few ulp, far below the decision margins of real trajectories
//      (tests/traj_actions_ref.py measures them).
// The loop stops once max_actions entries exist (every iteration that does not end the loop appends at least one), so it is bounded; the host list is
// reproduced up to that length. Latency-bound by design: 64 envs are 64 waves on 64 CUs, ~12 KB read per env.
#include "common.h"
#include "kernels.h"

#pragma clang fp contract(off)

namespace {

constexpr int kLanes = 64;
constexpr int kGroup = 32;          // samples per group: 32 x 2 coordinates = one chain per lane
constexpr int kChunk = 32;          // steps per chunk: 32 x 2 coordinates = one column per lane
constexpr int kRow = 66;            // floats per chunk row (64 chains + 2: column reads of consecutive steps fall in different banks)
constexpr int kMaxPoints = 1024;    // T + 1
constexpr int kMaxActions = 256;

constexpr double kStep = 0.25, kStopRadius = 0.2, kDegenerate = 1e-6;
constexpr double kTurn = 0x1.0c152382d7365p-2;    // np.deg2rad(15) = 15 * (pi / 180) in fp64
constexpr double kPi = 0x1.921fb54442d18p+1, kTwoPi = 0x1.921fb54442d18p+2;
constexpr int kLookAhead = 4;

template <typename T> __device__ __forceinline__ float load_scaled(const T* p);
template <> __device__ __forceinline__ float load_scaled<float>(const float* p) { return *p * 0.25f; }
// the host divides the bf16 tensor in place, then widens it: the product is rounded to bf16 first (it only rounds when it is subnormal)
template <> __device__ __forceinline__ float load_scaled<bf16>(const bf16* p) { return (float)(bf16)((float)*p * 0.25f); }

// (a + pi) % (2 pi) - pi with Python's %: fmod is exact, a non-zero remainder takes the divisor's (positive) sign
__device__ __forceinline__ double normalize_angle(double a) {
    double m = fmod(a + kPi, kTwoPi);
    if (m < 0.0) m += kTwoPi;
    else if (m == 0.0) m = 0.0;       // Python gives copysign(0, divisor) = +0
    return m - kPi;
}

__device__ __forceinline__ double norm2(double x, double y) { return sqrt(x * x + y * y); }

__device__ __forceinline__ double shfl_xor_f64(double v, int o) {
    int lo = __double2loint(v), hi = __double2hiint(v);
    lo = __shfl_xor(lo, o);
    hi = __shfl_xor(hi, o);
    return __hiloint2double(hi, lo);
}

// np.argmin order on (distance, index): a NaN is the minimum, then the smaller distance, then the lower index
__device__ __forceinline__ bool before(double d, int i, double od, int oi) {
    const bool n = d != d, on = od != od;
    if (n != on) return n;
    if (!n && d != od) return d < od;
    return i < oi;
}

template <typename T>
__global__ __launch_bounds__(kLanes) void traj_actions_kernel(T* __restrict__ traj, int S, int Tn, int32_t* __restrict__ actions, int max_actions,
                                                              int32_t* __restrict__ count, double* __restrict__ traj_out, int scale_in_place) {
    __shared__ double mean[kMaxPoints][2];
    __shared__ float cum[kChunk][kRow];
    __shared__ int32_t acts[kMaxActions];
    const int lane = threadIdx.x;
    const long b = blockIdx.x;
    const int P = Tn + 1;
    T* env = traj + b * S * Tn * 3;

    for (int i = lane; i < max_actions; i += kLanes) acts[i] = 0;
    if (lane < 2) mean[0][lane] = 0.0;

    // ---- 1 + 2: sequential fp32 sums per (sample, coordinate), sequential fp64 sum over the samples per (t, coordinate)
    const int cs = lane >> 1, cc = lane & 1;        // chain role: sample cs of the group, coordinate cc; column role: step cs of the chunk, coordinate cc
    for (int s0 = 0; s0 < S; s0 += kGroup) {
        const int ns = S - s0 < kGroup ? S - s0 : kGroup;
        T* row = env + ((long)(s0 + cs) * Tn) * 3 + cc;
        float run = 0.f;
        for (int t0 = 0; t0 < Tn; t0 += kChunk) {
            const int nt = Tn - t0 < kChunk ? Tn - t0 : kChunk;
            if (cs < ns) {
                for (int k = 0; k < nt; ++k) {
                    T* p = row + (long)(t0 + k) * 3;
                    const float v = load_scaled<T>(p);
                    if (scale_in_place) *p = (T)v;
                    run = (t0 + k == 0) ? v : run + v;          // np.cumsum starts from the first element (a -0 stays -0)
                    cum[k][lane] = run;
                }
            }
            __syncthreads();
            if (cs < nt) {
                double acc = s0 ? mean[1 + t0 + cs][cc] : (double)cum[cs][cc];
                for (int j = s0 ? 0 : 1; j < ns; ++j) acc += (double)cum[cs][j * 2 + cc];
                mean[1 + t0 + cs][cc] = acc;
            }
            __syncthreads();
        }
    }
    const double samples = (double)S;
    for (int i = 2 + lane; i < P * 2; i += kLanes) mean[i >> 1][i & 1] = mean[i >> 1][i & 1] / samples;
    __syncthreads();
    if (traj_out) {
        double* o = traj_out + b * P * 2;
        for (int i = lane; i < P * 2; i += kLanes) o[i] = mean[i >> 1][i & 1];
    }

    // ---- 3: pure pursuit (uniform over the wave; lane 0 records)
    const double gx = mean[P - 1][0], gy = mean[P - 1][1];
    double px = mean[0][0], py = mean[0][1], yaw = 0.0;
    int n = 0;
    while (n < max_actions) {
        const double dgoal = norm2(px - gx, py - gy);
        if (!(dgoal > kStopRadius)) break;
        double best = 0.0;
        int bi = P;                                   // P = no candidate yet (lanes beyond the last point)
        for (int i = lane; i < P; i += kLanes) {
            const double d = norm2(mean[i][0] - px, mean[i][1] - py);
            if (bi == P || before(d, i, best, bi)) { best = d; bi = i; }
        }
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) {
            const double od = shfl_xor_f64(best, o);
            const int oi = __shfl_xor(bi, o);
            if (oi < P && (bi == P || before(od, oi, best, bi))) { best = od; bi = oi; }
        }
        const int ti = bi + kLookAhead < P - 1 ? bi + kLookAhead : P - 1;
        const double tx = mean[ti][0] - px, ty = mean[ti][1] - py;
        if (norm2(tx, ty) < kDegenerate) break;
        const double turns = rint(normalize_angle(atan2(ty, tx) - yaw) / kTurn);
        if (!(fabs(turns) <= 64.0)) break;            // a NaN heading (the host raises there); |delta| <= pi gives at most 12
        const int nturns = (int)turns;
        const int code = nturns > 0 ? 2 : 3, reps = nturns > 0 ? nturns : -nturns;
        for (int k = 0; k < reps && n < max_actions; ++k, ++n)
            if (lane == 0) acts[n] = code;
        if (n >= max_actions) break;
        yaw = normalize_angle(yaw + (double)nturns * kTurn);
        const double nx = px + kStep * cos(yaw), ny = py + kStep * sin(yaw);
        if (norm2(nx - gx, ny - gy) > dgoal) break;
        if (lane == 0) acts[n] = 1;
        ++n;
        px = nx;
        py = ny;
    }
    __syncthreads();
    for (int i = lane; i < max_actions; i += kLanes) actions[b * max_actions + i] = acts[i];
    if (lane == 0) count[b] = n;
}

}  // namespace

int ina_launch_traj_actions(void* traj, int traj_dtype, int B, int S, int T, int32_t* actions, int max_actions, int32_t* count, double* traj_out,
                            int scale_in_place, hipStream_t stream) {
    INA_REQUIRE(traj && actions && count, "traj_actions: null tensor (traj %p, actions %p, count %p)", traj, (void*)actions, (void*)count);
    INA_REQUIRE(B >= 1 && S >= 1 && T >= 1, "traj_actions: bad shape B=%d S=%d T=%d (each must be >= 1)", B, S, T);
    INA_REQUIRE(T + 1 <= kMaxPoints, "traj_actions: T + 1 = %d points, at most %d", T + 1, kMaxPoints);
    INA_REQUIRE(max_actions >= 1 && max_actions <= kMaxActions, "traj_actions: max_actions=%d outside 1..%d", max_actions, kMaxActions);
    INA_REQUIRE(traj_dtype == INA_DT_F32 || traj_dtype == INA_DT_BF16, "traj_actions: traj dtype code %d is neither f32 nor bf16", traj_dtype);
    const double elems = (double)B * S * T;
    InaProfScope prof(INA_PROF_ELEMENTWISE, elems * 4.0, elems * 3.0 * (traj_dtype == INA_DT_F32 ? 4.0 : 2.0) + (double)B * (max_actions + 1) * 4.0, stream);
    if (traj_dtype == INA_DT_F32)
        hipLaunchKernelGGL(traj_actions_kernel<float>, dim3(B), dim3(kLanes), 0, stream, reinterpret_cast<float*>(traj), S, T, actions, max_actions,
                           count, traj_out, scale_in_place);
    else
        hipLaunchKernelGGL(traj_actions_kernel<bf16>, dim3(B), dim3(kLanes), 0, stream, reinterpret_cast<bf16*>(traj), S, T, actions, max_actions,
                           count, traj_out, scale_in_place);
    INA_HIP_CHECK(hipGetLastError());
    return 0;
}
