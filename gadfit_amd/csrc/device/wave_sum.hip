// lane l reads lane l + N of its row of 16 (DPP row_shl:N; lanes that would read past the row get 0): the low levels of a wave tree
template <int N> static __device__ __forceinline__ double gfh_row_down(const double v) {
  const long long b = __double_as_longlong(v);
  const int lo = __builtin_amdgcn_update_dpp(0, (int)b, 0x100 | N, 0xf, 0xf, true);
  const int hi = __builtin_amdgcn_update_dpp(0, (int)(b >> 32), 0x100 | N, 0xf, 0xf, true);
  return __longlong_as_double(((long long)hi << 32) | (unsigned)lo);
}
// the wave tree t_l += t_(l+32), (l+16), (l+8), (l+4), (l+2), (l+1) -- lane 0 ends with the sum, the additions of the __shfl_down loop it
// replaces bit for bit -- with the four levels inside a row as DPP moves instead of trips through the LDS crossbar (ds_bpermute)
static __device__ __forceinline__ double gfh_wave_sum(double t) {
  t += __shfl_down(t, 32, 64);
  t += __shfl_down(t, 16, 64);
  t += gfh_row_down<8>(t); t += gfh_row_down<4>(t); t += gfh_row_down<2>(t); t += gfh_row_down<1>(t);
  return t;
}
