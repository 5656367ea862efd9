// unet_train_common.inc -- what speedup_train.hip (2-D) and segment_train.hip (3-D) share of the backward pass: the kernels that work
// on flat [C][n] data and do not know the dimension of the net.  Included inside each file's unnamed namespace, after
// unet_common.inc (stats_kernel's segments, fold_segments, fixed_sum.inc's tree).  Each file's header states the rule these kernels follow.
//   norm_backward_stats_kernel + norm_backward_kernel: instance norm + LeakyReLU, backward (float64 sums, dx rounded once);
//   wgrad_fold_kernel: the float32 partials of a weight gradient added in float64 in their order, scaled, rounded once, added;
//   bias_grad_kernel: the same for the sums of dY; adam_kernel: one update in float64 per element, each result rounded once.

// grad[e] += scale x the partials of e added in float64 in their order, rounded once
__global__ __launch_bounds__(256) void wgrad_fold_kernel(const float* part, int n_part, size_t n_w, float* grad, double scale) {
  const size_t e = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= n_w) return;
  double s = 0.0;
  for (int p = 0; p < n_part; ++p) s += (double)part[(size_t)p * n_w + e];
  grad[e] += (float)(s * scale);
}

// grad[c] += scale x sum of dY[c]: stats_kernel's float64 sums, folded in order
__global__ __launch_bounds__(256) void bias_grad_kernel(const double2* part, int S, int C, float* grad, double scale) {
  const int c = blockIdx.x * 256 + threadIdx.x;
  if (c < C) grad[c] += (float)(fold_segments(part + (size_t)c * S, S).x * scale);
}

// ------------------------------------------------------------------------------------- instance norm + LeakyReLU, backward
__device__ __forceinline__ double xhat_of(float y) { return y > 0.f ? (double)y : (double)y / (double)0.01f; }
__device__ __forceinline__ double dxhat_of(float y, float dy) { return y > 0.f ? (double)dy : (double)0.01f * (double)dy; }

// part[c][s] = (sum of d xh, sum of d xh xh) of segment s of channel c: stats_kernel's segments and tree
__global__ __launch_bounds__(256) void norm_backward_stats_kernel(const float* y, const float* dy, size_t hw, int S, double2* part) {
  const int c = blockIdx.y, s = blockIdx.x, tid = threadIdx.x;
  const Segment g = segment_of(hw, S, s);
  const float* py = y + (size_t)c * hw;
  const float* pd = dy + (size_t)c * hw;
  double a = 0.0, b = 0.0;
  for (size_t i = g.lo + tid; i < g.hi; i += 256) {
    const double d = dxhat_of(py[i], pd[i]);
    a += d;
    b += d * xhat_of(py[i]);
  }
  const Sums<2> total = block_tree(Sums<2>{{a, b}});
  if (tid == 0) part[(size_t)c * S + s] = make_double2(total.v[0], total.v[1]);
}

// dy <- dx, in place; fpart: the forward's sums of the layer (mean, rstd), bpart: norm_backward_stats_kernel's
__global__ __launch_bounds__(256) void norm_backward_kernel(const float* y, float* dy, size_t hw, int S, const double2* fpart, const double2* bpart) {
  __shared__ double s_rstd, s_m1, s_m2;
  const int c = blockIdx.y;
  if (threadIdx.x == 0) {
    const double2 t = fold_segments(fpart + (size_t)c * S, S);
    const double m = t.x / (double)hw, var = fmax(t.y / (double)hw - m * m, 0.0);
    s_rstd = 1.0 / sqrt(var + 1e-5);
    const double2 b = fold_segments(bpart + (size_t)c * S, S);
    s_m1 = b.x / (double)hw;
    s_m2 = b.y / (double)hw;
  }
  __syncthreads();
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= hw) return;
  const size_t j = (size_t)c * hw + i;
  dy[j] = (float)(s_rstd * (dxhat_of(y[j], dy[j]) - s_m1 - xhat_of(y[j]) * s_m2));
}

// ---------------------------------------------------------------------------------------------------------------------- Adam
// step_size = lr / (1 - b1^t), inv_sqrt_bc2 = 1 / sqrt(1 - b2^t)
__global__ __launch_bounds__(256) void adam_kernel(float* w, const float* g, float* m1, float* m2, size_t n, double b1, double b2, double step_size,
                                                   double inv_sqrt_bc2) {
  const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const double gv = g[i];
  const double a = b1 * (double)m1[i] + (1.0 - b1) * gv, b = b2 * (double)m2[i] + (1.0 - b2) * gv * gv;
  m1[i] = (float)a;
  m2[i] = (float)b;
  w[i] = (float)((double)w[i] - step_size * a / (sqrt(b) * inv_sqrt_bc2 + 1e-8));
}

// ------------------------------------------------------------------------------------------------------------------ launches
void launch_norm_backward(const float* y, float* dy, int C, size_t n, const double2* fpart, double2* bpart) {
  const int S = segments_of(n);
  hipLaunchKernelGGL(norm_backward_stats_kernel, dim3((unsigned)S, (unsigned)C), dim3(256), 0, nullptr, y, dy, n, S, bpart);
  hipLaunchKernelGGL(norm_backward_kernel, dim3(blocks_of(n), (unsigned)C), dim3(256), 0, nullptr, y, dy, n, S, fpart, bpart);
}

// grad_w [n_w] += scale x its n_part partials; grad_b [c_out] += scale x the sums of dY [c_out][n] when grad_b (d_sums: room for them)
void launch_wgrad_fold(const float* part, int n_part, size_t n_w, float* grad_w, const float* dy, int c_out, size_t n, double2* d_sums, float* grad_b,
                       double scale) {
  hipLaunchKernelGGL(wgrad_fold_kernel, dim3(blocks_of(n_w)), dim3(256), 0, nullptr, part, n_part, n_w, grad_w, scale);
  if (grad_b) {
    hipLaunchKernelGGL(stats_kernel, dim3((unsigned)segments_of(n), (unsigned)c_out), dim3(256), 0, nullptr, dy, n, segments_of(n), d_sums);
    hipLaunchKernelGGL(bias_grad_kernel, dim3(blocks_of((size_t)c_out)), dim3(256), 0, nullptr, d_sums, segments_of(n), c_out, grad_b, scale);
  }
}

void launch_adam(float* w, const float* g, float* m1, float* m2, size_t n, double lr, double b1, double b2, unsigned long long t) {
  const double step_size = lr / (1.0 - std::pow(b1, (double)t)), inv_sqrt_bc2 = 1.0 / std::sqrt(1.0 - std::pow(b2, (double)t));
  hipLaunchKernelGGL(adam_kernel, dim3(blocks_of(n)), dim3(256), 0, nullptr, w, g, m1, m2, n, b1, b2, step_size, inv_sqrt_bc2);
}
