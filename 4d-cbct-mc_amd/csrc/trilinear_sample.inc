// trilinear_sample.inc -- the trilinear sampler that registration.hip and field_inverse.hip share: a volume [n0][n1][n2] (axis 2 the
// fastest in memory) at a float32 position, coordinate clamp, base index floor(c), upper tap clamped, blend a + (b - a) t along axis 2,
// then 1, then 0.  Every operation is rounded to float32; the including file is built with -ffp-contract=off.  Included inside the
// file's anonymous namespace, after <hip/hip_runtime.h>.
struct Shape {
  int n0, n1, n2;
  __host__ __device__ size_t voxels() const { return (size_t)n0 * n1 * n2; }
};

__device__ __forceinline__ float lerp(float a, float b, float t) { return a + (b - a) * t; }

// c clamped to [0, n - 1] (a NaN goes to 0), split into base index, upper index and fraction
__device__ __forceinline__ void split(float c, int n, int& lo, int& hi, float& t) {
  c = fminf(fmaxf(c, 0.f), (float)(n - 1));
  const float f = floorf(c);
  lo = (int)f;
  hi = min(lo + 1, n - 1);
  t = c - f;
}

__device__ __forceinline__ float blend8(const float* __restrict__ v, const Shape s, int a0, int b0, float t0, int a1, int b1, float t1, int a2, int b2, float t2) {
  const float* __restrict__ r00 = v + ((size_t)a0 * s.n1 + a1) * s.n2;
  const float* __restrict__ r01 = v + ((size_t)a0 * s.n1 + b1) * s.n2;
  const float* __restrict__ r10 = v + ((size_t)b0 * s.n1 + a1) * s.n2;
  const float* __restrict__ r11 = v + ((size_t)b0 * s.n1 + b1) * s.n2;
  const float x00 = lerp(r00[a2], r00[b2], t2), x01 = lerp(r01[a2], r01[b2], t2);
  const float x10 = lerp(r10[a2], r10[b2], t2), x11 = lerp(r11[a2], r11[b2], t2);
  return lerp(lerp(x00, x01, t1), lerp(x10, x11, t1), t0);
}

__device__ __forceinline__ float sample(const float* __restrict__ v, const Shape s, float c0, float c1, float c2) {
  int a0, b0, a1, b1, a2, b2;
  float t0, t1, t2;
  split(c0, s.n0, a0, b0, t0);
  split(c1, s.n1, a1, b1, t1);
  split(c2, s.n2, a2, b2, t2);
  return blend8(v, s, a0, b0, t0, a1, b1, t1, a2, b2, t2);
}

__device__ __forceinline__ bool voxel_of(size_t i, const Shape s, int& i0, int& i1, int& i2) {
  if (i >= s.voxels()) return false;
  const unsigned int v = (unsigned int)i, row = v / (unsigned int)s.n2;  // fewer than 2^31 voxels: 32-bit division
  i2 = (int)(v - row * (unsigned int)s.n2);
  i0 = (int)(row / (unsigned int)s.n1);
  i1 = (int)(row - (unsigned int)i0 * (unsigned int)s.n1);
  return true;
}
