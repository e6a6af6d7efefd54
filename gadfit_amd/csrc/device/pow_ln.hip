
// x**a and ln x from ONE extended-precision logarithm.  The device library's pow is 226 VALU instructions (28 of them selects
// on special cases), its log 98, and the derivative code of x**a wants both -- at every Kronrod node of every bisection of
// a quadrature model.  Here: x = 2^e m with m in [sqrt(1/2), sqrt(2)), s = (m - 1) / (m + 1) as a double-double (the
// quotient corrected by its own residual), ln m = 2 s + s z (2/3 + 2 z / 5 + ... + 2 z^9 / 21), z = s^2 (the truncation is
// below 2^-60 of the result for |s| <= 0.1716); ln x = e ln 2 + ln m summed as a double-double; x**a = exp(a ln x) with the
// low part of the product applied to first order.  About 90 VALU instructions for both results; measured against 60-digit
// references (tests/test_gpu_parity.py, test_device_pow_accuracy): <= 3 ulp (1.3 from the logarithm and the product, the rest gfh_exp) for |a ln x| <= 700 and 2^-1022 <= x < inf.
// Everything else -- x <= 0, subnormal, inf, NaN, overflowing exponents -- takes the library's pow and log, whose special
// cases are the reference's (IEEE pow).
static __device__ __forceinline__ double gfh_pow_ln(const double x, const double a, double& lnx) {
  if (x >= 0x1p-1022 && x < __builtin_inf()) {
    int e = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);                    // [0.5, 1)
    if (m < 0x1.6a09e667f3bcdp-1) { m = m + m; e -= 1; }         // [sqrt(1/2), sqrt(2))
    const double f = m - 1.0;                                      // exact
    const double dh = 2.0 + f, dl = (2.0 - dh) + f;               // m + 1 as a double-double
    double g = __builtin_amdgcn_rcp(dh);
    g = __builtin_fma(__builtin_fma(-dh, g, 1.0), g, g);
    g = __builtin_fma(__builtin_fma(-dh, g, 1.0), g, g);
    const double sh = f * g;
    const double sl = __builtin_fma(-sh, dl, __builtin_fma(-sh, dh, f)) * g;
    const double z = sh * sh;
    double p = __builtin_fma(z, 0x1.8618618618618p-4, 0x1.af286bca1af28p-4);      // 2/21, 2/19
    p = __builtin_fma(z, p, 0x1.e1e1e1e1e1e1ep-4);                                  // 2/17
    p = __builtin_fma(z, p, 0x1.1111111111111p-3);                                  // 2/15
    p = __builtin_fma(z, p, 0x1.3b13b13b13b14p-3);                                  // 2/13
    p = __builtin_fma(z, p, 0x1.745d1745d1746p-3);                                  // 2/11
    p = __builtin_fma(z, p, 0x1.c71c71c71c71cp-3);                                  // 2/9
    p = __builtin_fma(z, p, 0x1.2492492492492p-2);                                  // 2/7
    p = __builtin_fma(z, p, 0x1.999999999999ap-2);                                  // 2/5
    p = __builtin_fma(z, p, 0x1.5555555555555p-1);                                  // 2/3
    const double mh = sh + sh;
    const double ml = __builtin_fma(sh * z, p, sl + sl);                           // ln m = mh + ml
    const double ed = (double)e;
    const double th = ed * 0x1.62e42fee00000p-1;                                    // e ln2_hi: exact (ln2_hi carries 32 trailing zero bits)
    const double lh = th + mh;
    const double bb = lh - th;
    const double le = (th - (lh - bb)) + (mh - bb);                                // two-sum: th + mh = lh + le
    const double ll = __builtin_fma(ed, 0x1.a39ef35793c76p-33, le + ml);           // + e ln2_lo
    const double nh = lh + ll, nl = ll - (nh - lh);                                // renormalised: ln x = nh + nl, |nl| <= ulp(nh) / 2
    lnx = nh;
    const double ph = a * nh;
    const double pl = __builtin_fma(a, nl, __builtin_fma(a, nh, -ph));
    if (__builtin_fabs(ph) < 700.0) {
      const double r = gfh_exp(ph);
      return __builtin_fma(r, pl, r);
    }
  }
  lnx = log(x);
  return pow(x, a);
}
