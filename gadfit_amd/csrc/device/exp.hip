
// exp(x): the operations of the device library's exp (ROCm device-libs, __ocml_exp_f64: n = rint(x log2 e), two-step
// Cody-Waite reduction, its degree-11 polynomial, ldexp), so the same bits for every x that is not a NaN.  What differs
// is how the ends of the range are handled: the library computes ldexp(p, n) and then SELECTS +inf for x > 1024 and 0 for
// x < -1075 -- two v_cmp_f64 and three v_cndmask_b32 per call, and a v_cndmask_b32 that takes its mask from VCC costs
// 16-18 cycles per wave on gfx950 against 4-5 for an FP64 multiply-add (tools/microbench/fp64_rates.hip): a third of the
// call.  Here x is clamped to [-1075, 1024] first (two full-rate instructions; ldexp then overflows to +inf and
// underflows to 0 by itself, at the same x), and the one thing a clamp loses -- a NaN argument -- is put back with a
// compare into an SGPR pair and a select on the high word that takes its mask from there (4-5 cycles each).
typedef int int2_t_ __attribute__((ext_vector_type(2)));
static __device__ __forceinline__ double gfh_exp(const double x) {
  const double xc = __builtin_fmin(__builtin_fmax(x, -1075.0), 1024.0);
  const double dn = __builtin_rint(xc * 0x1.71547652b82fep+0);
  double r = __builtin_fma(-dn, 0x1.62e42fefa39efp-1, xc);
  r = __builtin_fma(-dn, 0x1.abc9e3b39803fp-56, r);
  double p = __builtin_fma(r, 0x1.ade156a5dcb37p-26, 0x1.28af3fca7ab0cp-22);
  p = __builtin_fma(r, p, 0x1.71dee623fde64p-19);
  p = __builtin_fma(r, p, 0x1.a01997c89e6b0p-16);
  p = __builtin_fma(r, p, 0x1.a01a014761f6ep-13);
  p = __builtin_fma(r, p, 0x1.6c16c1852b7b0p-10);
  p = __builtin_fma(r, p, 0x1.1111111122322p-7);
  p = __builtin_fma(r, p, 0x1.55555555502a1p-5);
  p = __builtin_fma(r, p, 0x1.5555555555511p-3);
  p = __builtin_fma(r, p, 0x1.000000000000bp-1);
  p = __builtin_fma(r, p, 1.0);
  p = __builtin_fma(r, p, 1.0);
  int2_t_ z = __builtin_bit_cast(int2_t_, __builtin_ldexp(p, (int)dn));
  unsigned long long is_nan;
  asm("v_cmp_u_f64 %0, %1, %1" : "=s"(is_nan) : "v"(x));
  int hi = z.y;
  asm("v_cndmask_b32 %0, %1, %2, %3" : "=v"(hi) : "v"(hi), "v"(0x7ff80000), "s"(is_nan));
  z.y = hi;
  return __builtin_bit_cast(double, z);
}
