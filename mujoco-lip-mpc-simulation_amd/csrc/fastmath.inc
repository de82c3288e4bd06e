// fastmath.inc — compact fp64 sincos / atan / atan2 / log for the interior-point kernels.
// Included by alipmpc.hip inside namespace alip, after rcp_nr.
// ---- compact fp64 transcendentals (fdlibm's published algorithms and minimax coefficients, written out here): the
// ocml versions are 3-5x larger and every copy in the hot loop costs instruction issue on every pass.  fp32 uses the
// ocml single-precision functions.
//
// Accuracy, in ulp of the correctly rounded result, measured on the MI355X against a 200-bit reference
// (tests/test_fastmath_gpu.py, profiles/fastmath/ulp.txt; in brackets the bar the test holds), and the domain each
// function is correct on.  Outside it the values below are what the code returns, not libm's; nothing in the solver
// reaches them (angles are headings, quotients come from coordinate differences of metre-sized numbers).
//   rcp_div(y, x)   0.50 [1.5] (fp32 0.50 [0.5]).  1 / x and y / x within the normal range.  Where 1 / x or the
//                   quotient overflows, x = +-0 or x = +-inf: NaN (rcp_nr, or inf * 0 in the correction).
//   div100(x)       0.48 [1.5] (fp32 0.48 [0.5]).  Every x whose x / 100 is normal.
//   lsincos(x)      sin 1.30, cos 1.37 [2.0] away from the multiples of pi/2.  The two-constant Cody-Waite reduction
//                   leaves an absolute error of |k| C, k = rint(x 2/pi), C = |pi/2 - hi - lo| = 1.4973849e-33, so
//                   the bound is |err| <= 2.0 ulp + |k| C: at the double nearest a multiple of pi/2 that is 451 ulp
//                   of the tiny result for |k| <= 64 and 548 ulp among 2000 random |k| <= 6.4e5 (0.996 of the
//                   bound both times) — below 1e-27 in absolute terms.  Domain |x| < 1e6 (denormals and +-0
//                   included).  lsincos(-0.0) returns +0 for the sine (k = -0, and (+0) + (-0) = +0 in the
//                   reduction).  |x| >= 1e6: |k| C keeps growing, and from |k| >= 2^31 the quadrant (int)k is wrong.
//                   +-inf, NaN: NaN.
//   latan(x)        0.78 [1.5].  x >= 0, +inf included (pi/2); x = NaN: NaN; x < 0 is not handled.
//   latan2(y, x)    1.30 [2.0].  Finite arguments whose quotient |y / x| and 1 / |x| are within the normal range, and
//                   the axes: (+-0, x > 0) -> +-0, (+-0, x < 0) -> +-pi, (y != 0, +-0) -> +-pi/2, (+-0, +0) -> +-0.
//                   latan2(+-0, -0.0) is +-0 where libm has +-pi.  Where 1 / |x| or the quotient overflows (latan2(1,
//                   1e-310), latan2(1e200, 1e-200)) or an argument is infinite: NaN (rcp_div), where libm has +-pi/2,
//                   +-0, +-pi or a multiple of pi/4.
//   llog(x)         0.66 [1.5].  x > 0 finite, denormals included; +-0 -> -inf, x < 0 or NaN -> NaN, +inf -> +inf.
// lsincos = lsincos_sel, latan = latan_br and latan2 = latan2_br bit for bit on every argument of those sets.
__device__ __forceinline__ double rcp_div(double y, double x)   // y / x (0.50 ulp measured, see above)
{
    const double r = rcp_nr(x);
    const double q = y * r;
    return fma(r, fma(-q, x, y), q);
}
__device__ __forceinline__ float rcp_div(float y, float x)
{
    const float r = rcp_nr(x);
    const float q = y * r;
    return fmaf(r, fmaf(-q, x, y), q);
}
// x / 100 (0.48 ulp measured; the scaling of IPOPT's s_max = 100): the product with 0.01 and its residual correction
__device__ __forceinline__ double div100(double x)
{
    const double q = x * 0.01;
    return fma(fma(-q, 100.0, x), 0.01, q);
}
__device__ __forceinline__ float div100(float x)
{
    const float q = x * 0.01f;
    return fmaf(fmaf(-q, 100.0f, x), 0.01f, q);
}
#ifdef ALIP_LIBM_MATH   // dev A/B: the ocml functions instead
__device__ __forceinline__ void lsincos(double x, double* sp, double* cp) { sincos(x, sp, cp); }
__device__ __forceinline__ double latan2(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ double latan2_br(double y, double x) { return atan2(y, x); }
__device__ __forceinline__ float latan2_br(float y, float x) { return atan2f(y, x); }
__device__ __forceinline__ double llog(double x) { return log(x); }
__device__ __forceinline__ void lsincos(float x, float* sp, float* cp) { sincosf(x, sp, cp); }
__device__ __forceinline__ void lsincos_sel(double x, double* sp, double* cp) { sincos(x, sp, cp); }
__device__ __forceinline__ void lsincos_sel(float x, float* sp, float* cp) { sincosf(x, sp, cp); }
__device__ __forceinline__ float latan2(float y, float x) { return atan2f(y, x); }
#else
// SIGNBIT: the quadrant signs by flipping the sign bit (the wave program: no selects between negated copies) or by
// selects (the lane program, lsincos_sel: the bit form had cost its register allocator 26 more spilled VGPRs, and
// cfg4 10.3 -> 11.7 ms).  The same bits either way.
template <bool SIGNBIT>
__device__ __forceinline__ void lsincos_t(double x, double* sp, double* cp)
{
    // x = k pi/2 + r, |r| <= pi/4 (Cody-Waite with FMA; |x| here is a heading angle, far below 1e6)
    const double k = rint(x * 0.63661977236758138243);
    double r = fma(-k, 1.57079632679489655800e+00, x);
    r = fma(-k, 6.12323399573676603587e-17, r);
    const double z = r * r;
    const double sp_ = fma(z, fma(z, fma(z, fma(z, fma(z, 1.58969099521155010221e-10, -2.50507602534068634195e-08),
                                                      2.75573137070700676789e-06), -1.98412698298579493134e-04),
                                     8.33333333332248946124e-03), -1.66666666666666324348e-01);
    const double sn = fma(r * z, sp_, r);
    const double cp_ = fma(z, fma(z, fma(z, fma(z, fma(z, -1.13596475577881948265e-11, 2.08757232129817482790e-09),
                                                      -2.75573143513906633035e-07), 2.48015872894767294178e-05),
                                     -1.38888888888741095749e-03), 4.16666666666666019037e-02);
    const double hz = 0.5 * z, w = 1.0 - hz;
    // (explicit fma wherever a product meets a sum: every kernel contracts these functions alike)
    const double cs = w + fma(z * z, cp_, (1.0 - w) - hz);
    const int q = (int)k & 3;
    const double s0 = (q & 1) ? cs : sn, c0 = (q & 1) ? sn : cs;
    if constexpr (SIGNBIT) {
        *sp = __hiloint2double(__double2hiint(s0) ^ ((q & 2) << 30), __double2loint(s0));
        *cp = __hiloint2double(__double2hiint(c0) ^ (((q + 1) & 2) << 30), __double2loint(c0));
    } else {
        *sp = (q & 2) ? -s0 : s0;
        *cp = ((q + 1) & 2) ? -c0 : c0;
    }
}
__device__ __forceinline__ void lsincos(double x, double* sp, double* cp) { lsincos_t<true>(x, sp, cp); }
__device__ __forceinline__ void lsincos_sel(double x, double* sp, double* cp) { lsincos_t<false>(x, sp, cp); }
__device__ __forceinline__ void lsincos(float x, float* sp, float* cp) { sincosf(x, sp, cp); }
__device__ __forceinline__ void lsincos_sel(float x, float* sp, float* cp) { sincosf(x, sp, cp); }

__device__ __forceinline__ double latan(double x)   // x >= 0 (incl. +inf)
{
    // fdlibm's argument reduction t = (a x + b) / (c x + d) on 5 intervals, branch-free: the interval's constants
    // are selected and ONE division runs (divergent lanes had executed every interval's division)
    const int id = x < 0.4375 ? -1 : x < 0.6875 ? 0 : x < 1.1875 ? 1 : x < 2.4375 ? 2 : 3;
    const double ca = id == 0 ? 2.0 : id == 3 ? 0.0 : 1.0;
    const double cb = id < 0 ? 0.0 : id == 0 ? -1.0 : id == 1 ? -1.0 : id == 2 ? -1.5 : -1.0;
    const double cc = id < 0 ? 0.0 : id == 2 ? 1.5 : 1.0;
    const double cd = id < 0 ? 1.0 : id == 0 ? 2.0 : id == 1 ? 1.0 : id == 2 ? 1.0 : 0.0;
    const double t = id < 0 ? x : (x == INFINITY ? -0.0 : rcp_div(fma(ca, x, cb), fma(cc, x, cd)));
    const double z = t * t, w = z * z;
    const double s1 = z * fma(w, fma(w, fma(w, fma(w, fma(w, 1.62858201153657823623e-02, 4.97687799461593236017e-02),
                                                    6.66107313738753120669e-02), 9.09088713343650656196e-02),
                                     1.42857142725034663711e-01), 3.33333333333329318027e-01);
    const double s2 = w * fma(w, fma(w, fma(w, fma(w, -3.65315727442169155270e-02, -5.83357013379057348645e-02),
                                            -7.69187620504482999495e-02), -1.11111104054623557880e-01),
                              -1.99999999998764832476e-01);
    const double hi = id == 0 ? 4.63647609000806093515e-01 : id == 1 ? 7.85398163397448278999e-01
                    : id == 2 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
    const double lo = id == 0 ? 2.26987774529616870924e-17 : id == 1 ? 3.06161699786838301793e-17
                    : id == 2 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
    const double sw = s1 + s2;
    return id < 0 ? fma(-t, sw, t) : hi - (fma(t, sw, -lo) - t);
}
__device__ __forceinline__ double latan_br(double x)   // x >= 0 (incl. +inf): the interval chain as branches
{
    // (the lane program keeps this form: with one instance per lane its registers, not divergence, set the pace — the
    // branch-free form measured 12 % slower there, cfg4 10.28 -> 11.51 ms)
    int id;
    double t;
    if (x < 0.4375) {
        id = -1; t = x;
    } else if (x < 0.6875) {
        id = 0; t = rcp_div(2.0 * x - 1.0, 2.0 + x);
    } else if (x < 1.1875) {
        id = 1; t = rcp_div(x - 1.0, x + 1.0);
    } else if (x < 2.4375) {
        id = 2; t = rcp_div(x - 1.5, fma(1.5, x, 1.0));
    } else {
        id = 3; t = x == INFINITY ? -0.0 : rcp_div(-1.0, x);
    }
    // (each interval's t is the branch-free latan's expression: the lane and wave programs round atan2 alike)
    const double z = t * t, w = z * z;
    const double s1 = z * fma(w, fma(w, fma(w, fma(w, fma(w, 1.62858201153657823623e-02, 4.97687799461593236017e-02),
                                                    6.66107313738753120669e-02), 9.09088713343650656196e-02),
                                     1.42857142725034663711e-01), 3.33333333333329318027e-01);
    const double s2 = w * fma(w, fma(w, fma(w, fma(w, -3.65315727442169155270e-02, -5.83357013379057348645e-02),
                                            -7.69187620504482999495e-02), -1.11111104054623557880e-01),
                              -1.99999999998764832476e-01);
    const double hi = id == 0 ? 4.63647609000806093515e-01 : id == 1 ? 7.85398163397448278999e-01
                    : id == 2 ? 9.82793723247329054082e-01 : 1.57079632679489655800e+00;
    const double lo = id == 0 ? 2.26987774529616870924e-17 : id == 1 ? 3.06161699786838301793e-17
                    : id == 2 ? 1.39033110312309984516e-17 : 6.12323399573676603587e-17;
    const double sw = s1 + s2;
    return id < 0 ? fma(-t, sw, t) : hi - (fma(t, sw, -lo) - t);
}
__device__ __forceinline__ double latan2(double y, double x)
{
    const double ax = fabs(x), ay = fabs(y);
    // (atan2(0, 0) = 0 as libm: argument 0; x = 0 < |y|: +inf)
    const double a = latan(ay == 0.0 ? 0.0 : ax == 0.0 ? INFINITY : rcp_div(ay, ax));
    const double b = x < 0.0 ? (3.14159265358979311600e+00 - a) + 1.22464679914735317720e-16 : a;
    return copysign(b, y);
}
__device__ __forceinline__ float latan2(float y, float x) { return atan2f(y, x); }

__device__ __forceinline__ double latan2_br(double y, double x)   // latan2 on latan_br (lane program)
{
    const double ax = fabs(x), ay = fabs(y);
    const double a = latan_br(ay < ax ? rcp_div(ay, ax) : (ax == 0.0 ? (ay == 0.0 ? 0.0 : INFINITY) : rcp_div(ay, ax)));
    const double b = x < 0.0 ? (3.14159265358979311600e+00 - a) + 1.22464679914735317720e-16 : a;
    return copysign(b, y);
}
__device__ __forceinline__ float latan2_br(float y, float x) { return atan2f(y, x); }

__device__ __forceinline__ double llog(double x)   // x > 0 finite; 0 -> -inf, x < 0 / NaN -> NaN, inf -> inf
{
    int e = __builtin_amdgcn_frexp_exp(x);
    double m = __builtin_amdgcn_frexp_mant(x);   // [0.5, 1)
    const bool lo = m < 0.70710678118654752440;
    m = lo ? m + m : m;
    e = lo ? e - 1 : e;
    const double f = m - 1.0;
    const double sv = rcp_div(f, 2.0 + f), z = sv * sv, w = z * z;
    const double t1 = w * fma(w, fma(w, 1.531383769920937332e-01, 2.222219843214978396e-01), 3.999999999940941908e-01);
    const double t2 = z * fma(w, fma(w, fma(w, 1.479819860511658591e-01, 1.818357216161805012e-01),
                                     2.857142874366239149e-01), 6.666666666666735130e-01);
    const double R2 = t2 + t1, hfsq = 0.5 * f * f, de = (double)e;
    const double r = de * 6.93147180369123816490e-01 -
                     ((hfsq - fma(sv, hfsq + R2, de * 1.90821492927058770002e-10)) - f);
    return x > 0.0 && x < INFINITY ? r : (x == 0.0 ? -INFINITY : (x == INFINITY ? INFINITY : __builtin_nan("")));
}
#endif
__device__ __forceinline__ float llog(float x) { return logf(x); }

