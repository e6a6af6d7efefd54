
// ---- The cross-wave reducer of the 256-lane form of the batch kernels (GFH_BLANES 256: a workgroup of four waves per fit).  Emitted in
// front of batch_fit.hip in that form alone, so that the text of the 64- and 16-lane forms holds no LDS and no barrier.
#define GFH_BWG_NACC (GFH_NA * (GFH_NA + 1) / 2 + GFH_NA + 1)      // batch_fit.hip's GFH_BNACC: the sweep's accumulators, the widest reduction
static __device__ __forceinline__ double gfh_uni(const double v) {      // lane 0's value as a wave-uniform one
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_readfirstlane((int)b), hi = __builtin_amdgcn_readfirstlane((int)(b >> 32));
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// the four waves' partial sums of one reduction, [image][wave][value]: 2 x 4 x 45 doubles at 8 active parameters
__shared__ double gfh_b_img[2][4][GFH_BWG_NACC];
// The fit-wide sums of n per-lane values at once, the same bits in every lane of the fit: each wave reduces with gfh_wave_sum, lane 0
// of each wave writes the wave's partials, and after the barrier every lane adds the four partials of each value in wave order.
// (The other forms keep their value-by-value gfh_b_sum at the three call sites: routed through an array-wise helper they computed
// the same values but were scheduled otherwise, and their instructions are held fixed.)
// One barrier per reduction, whatever n.  `img` (0 or 1, the same in every wave: see the barrier invariant above gfh_k_fit_batch) names
// the LDS image this reduction uses, and the reductions of a kernel alternate between the two.  Why one barrier is enough: between a
// wave's reads of an image in reduction k and ANY wave's next write to that image, in reduction k + 2, lies the barrier of reduction
// k + 1; no wave passes it before every wave has arrived at it, a wave arrives only after its reads of reduction k have returned (it
// added them), and a wave writes in reduction k + 2 only after it has passed.  Likewise the writes of reduction k + 1 go to the other
// image than the reads of reduction k that a slower wave may still be making.  The compiler moves no LDS access across __syncthreads().
template <int N> static __device__ __forceinline__ void gfh_b_sum_n(const double (&t)[N], double (&out)[N], int& img) {
  static_assert(N <= GFH_BWG_NACC, "the LDS image holds GFH_BWG_NACC values per wave");
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  double (&im)[4][GFH_BWG_NACC] = gfh_b_img[img];
  double s[N];
#pragma unroll
  for (int k = 0; k < N; k++) s[k] = gfh_wave_sum(t[k]);          // lane 0 of the wave ends with the wave's sum
  if ((threadIdx.x & 63) == 0) {                                   // (encloses no barrier)
#pragma unroll
    for (int k = 0; k < N; k++) im[wave][k] = s[k];
  }
  __syncthreads();
#pragma unroll
  for (int k = 0; k < N; k++) out[k] = gfh_uni(((im[0][k] + im[1][k]) + im[2][k]) + im[3][k]);
  img ^= 1;
}
