// philox_normal.inc -- the counter-based draws of the samplers (speedup_net.hip: sample_kernel; primary_project.hip: the compound
// Poisson and Gaussian samplers).  Included inside the including file's unnamed namespace.
//   Block      Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3") with key (seed low word, seed high word)
//              and counter (x, y, projection, k): x, y the pixel's column and row in the plane, k the number of the draw at that pixel.
//   Uniforms   u1 = ((w0 >> 8) + 1) 2^-24 in (0, 1], u2 = (w1 >> 8) 2^-24 in [0, 1), of words 0 and 1 of the block.
//   Normal     z = sqrt(-2 ln u1) cos(2 pi u2) (Box-Muller): standard_normal in float32, normal_of_words in double.
__device__ void philox10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1, unsigned& w0, unsigned& w1) {
#pragma unroll
  for (int i = 0; i < 10; ++i) {
    const unsigned long long p0 = 0xD2511F53ull * c0, p1 = 0xCD9E8D57ull * c2;
    const unsigned n0 = (unsigned)(p1 >> 32) ^ c1 ^ k0, n2 = (unsigned)(p0 >> 32) ^ c3 ^ k1;
    c1 = (unsigned)p1;
    c3 = (unsigned)p0;
    c0 = n0;
    c2 = n2;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  w0 = c0;
  w1 = c1;
}

__device__ float standard_normal(int x, int y, unsigned projection, unsigned long long seed) {
  unsigned w0, w1;
  philox10((unsigned)x, (unsigned)y, projection, 0u, (unsigned)seed, (unsigned)(seed >> 32), w0, w1);
  const float u1 = (float)((w0 >> 8) + 1u) * 0x1p-24f, u2 = (float)(w1 >> 8) * 0x1p-24f;  // u1 in (0, 1], u2 in [0, 1)
  return sqrtf(-2.f * logf(u1)) * cospif(2.f * u2);
}

// the same mapping in double: u1 of word 0 (returned in `u`), the normal of words 0 and 1
__device__ __forceinline__ double normal_of_words(unsigned w0, unsigned w1, double& u) {
  u = (double)((w0 >> 8) + 1u) * 0x1p-24;
  return sqrt(-2.0 * log(u)) * cospi(2.0 * ((double)(w1 >> 8) * 0x1p-24));
}
