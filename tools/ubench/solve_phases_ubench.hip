// Micro-benchmarks behind the work on the phases AROUND the elimination of the 24-state solve (iekf_solve_body, lii_iekf.hip;
// profiles/solve_phases.md): what do the A-phase and the state phase cost a workgroup of 256 lanes that has the compute unit to itself
// and runs them with resident code (every block repeated, timed with s_memtime and s_memrealtime on the first wavefront)?
//   A-phase  1: as the library forms A = I + P11 G - one element per lane (144 lanes), the sum in k-order, A through LDS, barrier, every lane
//               of the elimination loads its column;  2: in the elimination's layout - every lane p < 12 of a 16-lane row builds column p
//               (twelve chains of twelve multiply-adds from broadcast reads), nothing handed over.
//   state    3: one wavefront, in the order the library had: schedule (two square roots on every lane), vector blocks, solution, then the
//               two rotations (boxplus over 2 x 9 lanes, two exchanges through LDS), stores;  4: the rotations first and alone, the
//               schedule behind their stores (the vector blocks, the solution and the control words on the other wavefronts);
//            5: the rotations alone;  6: the schedule alone.
// build: hipcc --offload-arch=gfx950 -O3 -ffp-contract=fast -o solve_phases_ubench solve_phases_ubench.hip ; run: ./solve_phases_ubench
#include <hip/hip_runtime.h>
#include <cstdio>
#include <vector>

constexpr int N = 24, H = 12, LDH = 13;

__device__ __forceinline__ double boxplus_rot_entry(const double* v, const double* R, double* xk, double* xck, double* xe, int e) {
#pragma clang fp contract(off)
  const int r = e / 3, cc = e % 3;
  const double v1 = v[0], v2 = v[1], v3 = v[2];
  const double n = sqrt(v1 * v1 + v2 * v2 + v3 * v3);
  const double id = (r == cc) ? 1.0 : 0.0;
  double E = id;
  if (n > 0.00001) {
    const double a = v[r == cc ? 0 : 3 - r - cc] / n;
    const double k = (r == cc) ? 0.0 : ((cc == (r + 1) % 3) ? -a : a);
    const double s = sin(n), c1 = 1.0 - cos(n);
    xk[e] = k;
    xck[e] = c1 * k;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    const double kk = xck[3 * r] * xk[cc] + xck[3 * r + 1] * xk[3 + cc] + xck[3 * r + 2] * xk[6 + cc];
    E = (id + s * k) + kk;
  }
  xe[e] = E;
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
  return R[3 * r] * xe[cc] + R[3 * r + 1] * xe[3 + cc] + R[3 * r + 2] * xe[6 + cc];
}

#define T0() do { __syncthreads(); __builtin_amdgcn_s_waitcnt(0); asm volatile("s_nop 0" ::: "memory"); c0 = __builtin_amdgcn_s_memtime(); r0 = __builtin_amdgcn_s_memrealtime(); } while (0)
#define T1(slot) do { __builtin_amdgcn_s_waitcnt(0); asm volatile("s_nop 0" ::: "memory"); c1 = __builtin_amdgcn_s_memtime(); r1 = __builtin_amdgcn_s_memrealtime(); if (threadIdx.x == 0) { out[2 * (slot)] = (long long)(c1 - c0); out[2 * (slot) + 1] = (long long)(r1 - r0); } } while (0)

__global__ __launch_bounds__(256) void k_bench(long long* out, double* sink, const double* src, double* gst, int reps) {
  __shared__ double s_cov[N * N], A[H * LDH], s_ne[96], sol[N], s_st[36], s_rx[2][3][9];
  unsigned long long c0, c1, r0, r1;
  const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
  for (int e = tid; e < N * N; e += 256) s_cov[e] = src[e] * 1e-3 + (e / N == e % N ? 1e-2 : 0.0);
  if (tid < 96) s_ne[tid] = src[600 + tid];
  if (tid < N) sol[tid] = 1e-3 * src[700 + tid];
  if (tid < 36) s_st[tid] = tid < 9 ? (tid % 4 == 0 ? 1.0 : 0.0) : (tid >= 12 && tid < 21 ? ((tid - 12) % 4 == 0 ? 1.0 : 0.0) : 0.5);  // two identity rotations
  __syncthreads();
  double acc = 0;
  T0(); T1(0);
  // 1: the library's A-phase
  T0();
  for (int it = 0; it < reps; it++) {
    if (tid < H * H) {
      const int i = tid / H, j = tid % H;
      double s = (i == j) ? 1.0 : 0.0;
#pragma unroll
      for (int k = 0; k < H; k++) {
        const int a = k < j ? k : j, b = k < j ? j : k;
        s += s_cov[i * N + k] * s_ne[a * H - (a * (a - 1)) / 2 + (b - a)];
      }
      A[i * LDH + j] = s;
    }
    __syncthreads();
    if (wave < 2) {
      const int p = lane & 15, j = 16 * wave + 4 * (lane >> 4) + (p - H);
      double col[H];
#pragma unroll
      for (int r = 0; r < H; r++) col[r] = p < H ? A[r * LDH + p] : (j < N ? s_cov[r * N + j] : 0.0);
#pragma unroll
      for (int r = 0; r < H; r++) acc += col[r];
    }
    __syncthreads();
    if (tid == 0) s_ne[0] += 1e-9;
  }
  T1(1);
  // 2: every lane of the elimination's layout builds its own column
  T0();
  for (int it = 0; it < reps; it++) {
    if (wave < 2) {
      const int p = lane & 15, j = 16 * wave + 4 * (lane >> 4) + (p - H);
      double col[H];
#pragma unroll
      for (int r = 0; r < H; r++) {
        if (p < H) {
          double s = (r == p) ? 1.0 : 0.0;
#pragma unroll
          for (int k = 0; k < H; k++) {
            const int a = k < p ? k : p, b = k < p ? p : k;
            s += s_cov[r * N + k] * s_ne[a * H - (a * (a - 1)) / 2 + (b - a)];
          }
          col[r] = s;
        } else {
          col[r] = j < N ? s_cov[r * N + j] : 0.0;
        }
      }
#pragma unroll
      for (int r = 0; r < H; r++) acc += col[r];
    }
    if (tid == 0) s_ne[0] += 1e-9;
    __syncthreads();
  }
  T1(2);
  // 3 - 6: the state phase on the first wavefront (the others wait at the barrier of the next T0)
  for (int form = 3; form <= 6; form++) {
    T0();
    if (wave == 0) {
      for (int it = 0; it < reps; it++) {
        int do_cov = 0;
        const bool rot_lane = lane < 32 && (lane & 15) < 9;
        const int rho = lane >> 4, e = lane & 15, o = 12 * rho;
        if (form == 3 || form == 6) {
          const double rn = sqrt(sol[0] * sol[0] + sol[1] * sol[1] + sol[2] * sol[2]);
          const double tn = sqrt(sol[3] * sol[3] + sol[4] * sol[4] + sol[5] * sol[5]);
          do_cov = (rn * 57.3 < 0.01) && (tn * 100 < 0.015);
        }
        if (form == 3) {
          if (lane >= 8 && lane < 26) {
            const int q = lane - 8;
            const double v = s_st[9 + q] + sol[3 + q];
            gst[64 + q] = v;
            if (do_cov) gst[128 + q] = v;
          } else if (lane >= 32 && lane < 32 + N) {
            gst[192 + lane] = sol[lane - 32];
          }
        }
        if (form != 6 && rot_lane) {
          const double v = boxplus_rot_entry(sol + 6 * rho, s_st + o, s_rx[rho][0], s_rx[rho][1], s_rx[rho][2], e);
          gst[o + e] = v;
          if (form == 3 && do_cov) gst[128 + o + e] = v;
        }
        if (form == 4) {
          const double rn = sqrt(sol[0] * sol[0] + sol[1] * sol[1] + sol[2] * sol[2]);
          const double tn = sqrt(sol[3] * sol[3] + sol[4] * sol[4] + sol[5] * sol[5]);
          do_cov = (rn * 57.3 < 0.01) && (tn * 100 < 0.015);
          if (rot_lane && do_cov) gst[128 + o + e] = 1.0;
        }
        acc += do_cov;
        if (lane == 0) sol[it & 7] += 1e-9;  // (the next repetition depends on this one)
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "wavefront");
      }
    }
    T1(form);
  }
  sink[tid] = acc;
}

#define CHK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("%s: %s\n", #x, hipGetErrorString(e_)); return 1; } } while (0)
int main() {
  long long* d_out; double *d_sink, *d_src, *d_gst;
  CHK(hipMalloc(&d_out, 64 * sizeof(long long))); CHK(hipMalloc(&d_sink, 256 * sizeof(double))); CHK(hipMalloc(&d_src, 1024 * 8)); CHK(hipMalloc(&d_gst, 512 * 8));
  std::vector<double> src(1024);
  for (size_t i = 0; i < src.size(); i++) src[i] = 1.0 + 0.001 * (double)(i % 97);
  CHK(hipMemcpy(d_src, src.data(), src.size() * 8, hipMemcpyHostToDevice));
  const char* names[7] = {"empty", "A-phase: element per lane, LDS, barrier, column loads", "A-phase: column per lane, no hand-over",
                          "state: schedule, vectors, solution, rotations", "state: rotations, then schedule", "state: rotations alone", "state: schedule alone"};
  for (int pass = 0; pass < 7; pass++) {
    const int reps = 100;
    hipLaunchKernelGGL(k_bench, dim3(1), dim3(256), 0, 0, d_out, d_sink, d_src, d_gst, reps);
    CHK(hipDeviceSynchronize());
    long long out[64];
    CHK(hipMemcpy(out, d_out, sizeof(out), hipMemcpyDeviceToHost));
    if (pass < 2) continue;  // (five timed runs: their spread is the cut-off for any comparison)
    printf("256 lanes, %d repetitions per block:\n", reps);
    for (int s = 0; s < 7; s++)
      printf("  %-56s %8.1f clk / rep  %7.1f ns / rep   (clock %.2f GHz)\n", names[s], (double)(out[2 * s] - out[0]) / reps, (double)(out[2 * s + 1] - out[1]) * 10.0 / reps,
             out[2 * s + 1] > out[1] ? (double)(out[2 * s] - out[0]) / ((double)(out[2 * s + 1] - out[1]) * 10.0) : 0.0);
  }
  return 0;
}
