// The bootstrapped Evaluator (training/evaluation.py:164-386) on per-molecule MOMENTS.  Every metric the reference takes over the
// concatenated tensors of a (resampled) dataset is a function of a handful of sums over its molecules, so a bootstrap replicate
// does not have to torch.cat thousands of per-molecule tensors: it gathers and adds rows of GRAPPA_EVAL_NMOM doubles.
//   eval_moments_kernel     one workgroup per molecule (as eval_se_kernel, loss.hip): fp32 inputs, double from the first subtraction on
//   eval_bootstrap_kernel   one workgroup per (dataset, replicate): gather rows, add them in a fixed order, finalise the 7 metrics
//   eval_spread_kernel      one workgroup per dataset: mean and population std of every metric over the replicates
// All sums are made in a fixed order (strided per-thread partials, butterfly over the 64 lanes, the four wavefronts in order); there
// is no atomic: the same input gives the same bits.
#include "common.h"

namespace {

constexpr int NMOM = GRAPPA_EVAL_NMOM;
constexpr int NMET = GRAPPA_EVAL_NMETRICS;
static_assert(NMOM == 10 && (NMOM * sizeof(double)) % 16 == 0, "a moment row is read as 16-byte pieces");

__device__ inline double wave_sum_d(double v) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
    return v;
}

// sums of K values per thread over the 256 threads of the workgroup; the result in every thread.  red: 4 * K doubles
template <int K> __device__ inline void block_sum_d(double (&v)[K], double* red) {
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = wave_sum_d(v[k]);
    __syncthreads();                       // (the previous call's readers are done with `red`)
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int k = 0; k < K; ++k) red[(threadIdx.x >> 6) * K + k] = v[k];
    }
    __syncthreads();
#pragma unroll
    for (int k = 0; k < K; ++k) v[k] = (red[k] + red[K + k]) + (red[2 * K + k] + red[3 * K + k]);
}

// out[b][0..4] = n_E, sum d^2, sum |d|, sum r, sum r^2 over the real conformations (d = centred prediction - centred reference,
// r = centred reference; centring per molecule over its real conformations, utils/graph_utils.py:35-63);
// out[b][5..9] = n_V = atoms x real conformations, sum |dg|^2, sum |dg| over the 3-vectors, sum and sum of squares of the reference's components.
// A dummy conformation is skipped, never multiplied by zero: whatever its slots hold (NaN included) stays out of the sums.
__global__ __launch_bounds__(256) void eval_moments_kernel(int B, int C, int N, const int* __restrict__ atom_molptr, const float* __restrict__ energy,
                                                           const float* __restrict__ energy_ref, const float* __restrict__ is_dummy,
                                                           const float* __restrict__ grad, const float* __restrict__ grad_ref,
                                                           double* __restrict__ out) {
    __shared__ double red[4 * 5];
    const int b = blockIdx.x, tid = threadIdx.x;
    const float* dm = is_dummy ? is_dummy + (size_t)b * C : nullptr;
    const float* e = energy + (size_t)b * C;
    const float* er = energy_ref + (size_t)b * C;
    double s[3] = {0.0, 0.0, 0.0};                      // real conformations, sum E, sum E_ref
    for (int c = tid; c < C; c += 256) {
        if (dm && dm[c] != 0.f) continue;
        s[0] += 1.0;
        s[1] += (double)e[c];
        s[2] += (double)er[c];
    }
    block_sum_d<3>(s, red);
    const double nreal = s[0], me = s[1] / nreal, mr = s[2] / nreal;
    double m[4] = {0.0, 0.0, 0.0, 0.0};                 // sum d^2, sum |d|, sum r, sum r^2
    for (int c = tid; c < C; c += 256) {
        if (dm && dm[c] != 0.f) continue;
        const double r = (double)er[c] - mr, d = ((double)e[c] - me) - r;
        m[0] += d * d;
        m[1] += fabs(d);
        m[2] += r;
        m[3] += r * r;
    }
    block_sum_d<4>(m, red);
    double g[4] = {0.0, 0.0, 0.0, 0.0};                 // sum |dg|^2, sum |dg|, sum g_ref, sum g_ref^2
    const int a0 = min(max(atom_molptr[b], 0), N), a1 = min(max(atom_molptr[b + 1], a0), N);      // (never beyond the N atoms of the tables)
    const bool with_grad = grad && grad_ref;
    if (with_grad) {
        const size_t base = (size_t)a0 * C * 3, nvec = (size_t)(a1 - a0) * C;
        for (size_t i = tid; i < nvec; i += 256) {       // one 3-vector (atom, conformation) per thread and turn
            if (dm && dm[i % C] != 0.f) continue;
            const float* p = grad + base + 3 * i;
            const float* q = grad_ref + base + 3 * i;
            const double q0 = q[0], q1 = q[1], q2 = q[2];
            const double d0 = (double)p[0] - q0, d1 = (double)p[1] - q1, d2 = (double)p[2] - q2;
            const double sq = d0 * d0 + d1 * d1 + d2 * d2;
            g[0] += sq;
            g[1] += sqrt(sq);
            g[2] += q0 + q1 + q2;
            g[3] += q0 * q0 + q1 * q1 + q2 * q2;
        }
        block_sum_d<4>(g, red);
    }
    if (tid == 0) {
        double2* row = reinterpret_cast<double2*>(out + (size_t)b * NMOM);        // rows are 80 bytes: 16-byte aligned with the buffer
        row[0] = make_double2(nreal, m[0]);
        row[1] = make_double2(m[1], m[2]);
        row[2] = make_double2(m[3], with_grad ? (double)(a1 - a0) * nreal : 0.0);
        row[3] = make_double2(g[0], g[1]);
        row[4] = make_double2(g[2], g[3]);
    }
}

__device__ inline double nonneg(double v) { return v < 0.0 ? 0.0 : v; }      // (a NaN stays a NaN)

// Workgroup (d, r): replicate rep0 + r of dataset d.  Its molecules are the rows ds_ptr[d] + idx[r][ds_ptr[d] + j], j < n_d: 80-byte rows
// read as five 16-byte pieces (a table of a few MB at most: after the first replicates it is served by L2 / the Infinity Cache).
// An index outside [0, n_d) is CLAMPED into the dataset (the entry point cannot look at device memory; see include/grappa_hip.h).
__global__ __launch_bounds__(256) void eval_bootstrap_kernel(const double* __restrict__ mom, int M, const int* __restrict__ ds_ptr,
                                                             const int* __restrict__ idx, int n_ds, int rep0, double* __restrict__ rep_metrics) {
    __shared__ double red[4 * NMOM];
    const int d = blockIdx.x, r = blockIdx.y, tid = threadIdx.x;
    const int p0 = min(max(ds_ptr[d], 0), M), n = min(max(ds_ptr[d + 1], p0), M) - p0;      // (never beyond the M rows of the tables)
    const int* sel = idx + (size_t)r * M + p0;
    double s[NMOM];
#pragma unroll
    for (int k = 0; k < NMOM; ++k) s[k] = 0.0;
    for (int j = tid; j < n; j += 256) {
        int k = sel[j];
        k = k < 0 ? 0 : (k >= n ? n - 1 : k);
        const double2* row = reinterpret_cast<const double2*>(mom + (size_t)(p0 + k) * NMOM);
#pragma unroll
        for (int q = 0; q < NMOM / 2; ++q) {
            const double2 v = row[q];
            s[2 * q] += v.x;
            s[2 * q + 1] += v.y;
        }
    }
    block_sum_d<NMOM>(s, red);
    if (tid == 0) {
        // get_metrics (training/evaluation.py:358-377), in its order.  A zero count divides 0 by 0: NaN, as torch's mean / std of nothing
        const double nE = s[0], nV = s[5], nC = 3.0 * s[5];
        double* o = rep_metrics + ((size_t)(rep0 + r) * n_ds + d) * NMET;
        o[0] = sqrt(nonneg(s[4] - s[3] * s[3] / nE) / (nE - 1.0));                      // std_energies (unbiased)
        o[1] = sqrt(nonneg(s[9] - s[8] * s[8] / nC) / (nC - 1.0)) * sqrt(3.0);          // std_gradients: all components, x sqrt(3)
        o[2] = sqrt(s[1] / nE);                                                         // rmse_energies
        o[3] = s[2] / nE;                                                               // mae_energies
        o[4] = sqrt(s[6] / nV);                                                         // rmse_gradients (per 3-vector)
        o[5] = sqrt(s[6] / nC);                                                         // crmse_gradients (per component)
        o[6] = s[7] / nV;                                                               // mae_gradients
    }
}

// mean and population std (np.std, training/evaluation.py:346) of every metric of dataset d over the n_rep replicates, two passes.  The
// values are taken relative to replicate 0 (the full dataset): replicates that are all equal -- a dataset of one molecule -- give that
// value as the mean and exactly 0 as the std, for every n_rep.
__global__ __launch_bounds__(256) void eval_spread_kernel(const double* __restrict__ rep_metrics, int n_rep, int n_ds, double* __restrict__ mean,
                                                          double* __restrict__ stdev) {
    __shared__ double red[4 * NMET];
    const int d = blockIdx.x, tid = threadIdx.x;
    const double* x = rep_metrics + (size_t)d * NMET;
    const size_t ld = (size_t)n_ds * NMET;
    double x0[NMET], s[NMET];
#pragma unroll
    for (int k = 0; k < NMET; ++k) {
        x0[k] = x[k];
        s[k] = 0.0;
    }
    for (int r = tid; r < n_rep; r += 256) {
#pragma unroll
        for (int k = 0; k < NMET; ++k) s[k] += x[r * ld + k] - x0[k];
    }
    block_sum_d<NMET>(s, red);
    double mu[NMET], q[NMET];
#pragma unroll
    for (int k = 0; k < NMET; ++k) {
        mu[k] = s[k] / (double)n_rep;
        q[k] = 0.0;
    }
    for (int r = tid; r < n_rep; r += 256) {
#pragma unroll
        for (int k = 0; k < NMET; ++k) {
            const double t = (x[r * ld + k] - x0[k]) - mu[k];
            q[k] += t * t;
        }
    }
    block_sum_d<NMET>(q, red);
    if (tid < NMET) {
        double m = 0.0, v = 0.0;
#pragma unroll
        for (int k = 0; k < NMET; ++k) {
            if (k == tid) {
                m = x0[k] + mu[k];
                v = sqrt(q[k] / (double)n_rep);
            }
        }
        mean[(size_t)d * NMET + tid] = m;
        stdev[(size_t)d * NMET + tid] = v;
    }
}

}  // namespace

extern "C" int grappa_eval_moments_f32(void* stream, int B, int C, int N, const int* atom_molptr, const float* energy, const float* energy_ref,
                                       const float* is_dummy, const float* grad, const float* grad_ref, double* out) {
    if (B <= 0 || C <= 0 || N < 0 || !atom_molptr || !energy || !energy_ref || !out) return GRAPPA_ERR_ARG;
    if ((grad == nullptr) != (grad_ref == nullptr)) return GRAPPA_ERR_ARG;
    if (reinterpret_cast<uintptr_t>(out) % 16 != 0) return GRAPPA_ERR_ARG;
    GRAPPA_LAUNCH(eval_moments_kernel, dim3(B), dim3(256), 0, reinterpret_cast<hipStream_t>(stream), B, C, N, atom_molptr, energy, energy_ref,
                  is_dummy, grad, grad_ref, out);
    return grappa_launch_status();
}

extern "C" int grappa_eval_bootstrap_f64(void* stream, const double* mom, int M, int n_ds, const int* ds_ptr, const int* idx, int n_rep, int rep0,
                                         int rep1, double* rep_metrics, double* mean, double* stdev) {
    if (!mom || !ds_ptr || !idx || !rep_metrics || !mean || !stdev) return GRAPPA_ERR_ARG;
    if (M < 1 || n_ds < 1 || n_rep < 1 || rep0 < 0 || rep1 <= rep0 || rep1 > n_rep) return GRAPPA_ERR_ARG;
    if (rep1 - rep0 > 65535) return GRAPPA_ERR_ARG;          // grid (n_ds, replicates of the call)
    if (reinterpret_cast<uintptr_t>(mom) % 16 != 0) return GRAPPA_ERR_ARG;
    hipStream_t st = reinterpret_cast<hipStream_t>(stream);
    GRAPPA_LAUNCH(eval_bootstrap_kernel, dim3(n_ds, rep1 - rep0), dim3(256), 0, st, mom, M, ds_ptr, idx, n_ds, rep0, rep_metrics);
    if (rep1 == n_rep)             // the last range: every replicate's metrics are written (stream order) -- their mean and spread
        GRAPPA_LAUNCH(eval_spread_kernel, dim3(n_ds), dim3(256), 0, st, rep_metrics, n_rep, n_ds, mean, stdev);
    return grappa_launch_status();
}
