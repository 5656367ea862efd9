// fixed_sum.inc -- the float64 sums that give the same bytes on every call (registration.hip, field_inverse.hip, wpc_fit.hip,
// rooster4d.hip, the U-Net statistics of unet_common.inc and unet_train_common.inc, the losses of speedup_train.hip and
// segment_train.hip).  Included inside each file's unnamed namespace, after hip_host.hpp.
//
// THE RULE.  No float atomics, and nothing that depends on the device or on the order in which blocks finish:
//   1. every thread adds its share in float64 in a fixed order (the kernel's own loop: rising index, the components of an item in order);
//   2. the 256 threads of a block combine their values by one tree: for h = 128, 64 .. 1, slot t < h takes slot t + h (block_tree);
//   3. the blocks' (or segments') partials are added in rising order, from 0.0, one after the other: on the host by fold_blocks, on
//      the device by the kernel that reads them (rooster4d.hip's sum_partials_kernel, fold_segments, dice_fold_kernel).
// tests/fixed_sum_ref.py restates 1 - 3 in numpy; tests/test_field_inverse_gpu.py and tests/test_registration_gpu.py hold two of the
// kernels to it with ==.

// ---- what a thread hands to the tree: a double, N doubles together, or a sum with a float maximum -------------------------------
template <int N>
struct Sums { double v[N]; };
struct SumMax { double sum; float top; };

__device__ __forceinline__ void combine(double& a, const double& b) { a += b; }
template <int N>
__device__ __forceinline__ void combine(Sums<N>& a, const Sums<N>& b) {
#pragma unroll
  for (int k = 0; k < N; ++k) a.v[k] += b.v[k];
}
__device__ __forceinline__ void combine(SumMax& a, const SumMax& b) {
  a.sum += b.sum;
  a.top = fmaxf(a.top, b.top);
}

// Step 2, for a block of 256 threads, all of which call it.  THREAD 0 gets the block's total; every other thread gets the partial
// result of its own slot, which means nothing.  All parts of V go through the one barrier sequence (nine barriers).
// Calling it again in the same kernel is safe and needs no barrier in between: after the last barrier a thread reads only its own
// slot, and the next call's first access to a slot is its owner's store, so every access between that barrier and the next call's
// first one is by the slot's owner, in program order.  (A form that hands lds[0] to all threads would need a barrier after that read.)
template <class V>
__device__ __forceinline__ V block_tree(const V& v) {
  __shared__ V lds[256];
  lds[threadIdx.x] = v;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if ((int)threadIdx.x < h) combine(lds[threadIdx.x], lds[threadIdx.x + h]);
    __syncthreads();
  }
  return lds[threadIdx.x];
}

// Step 3 on the host: d_partial is [blocks][terms] on the device; sum[t] = ((0.0 + partial[0][t]) + partial[1][t]) + ...
void fold_blocks(const double* d_partial, int blocks, int terms, double* sum) {
  std::vector<double> partial((size_t)blocks * terms);
  HIP_TRY(hipMemcpy(partial.data(), d_partial, partial.size() * sizeof(double), hipMemcpyDeviceToHost));
  for (int t = 0; t < terms; ++t) {
    sum[t] = 0.0;
    for (int b = 0; b < blocks; ++b) sum[t] += partial[(size_t)b * terms + t];
  }
}
