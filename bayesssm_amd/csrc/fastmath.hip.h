// fastmath.hip.h -- range-specialised forms of the device library functions on the filter kernels' issue-bound paths.
//
// k_obs's local phases (and k_step / k_weights of the multi-launch path) are bound by vector-instruction issue (DESIGN.md
// section 5f), and most of their instruction stream is general-purpose library code run on arguments whose range is known at
// compile time.  Every function here is the device library's OWN algorithm -- the same operations on the same constants in
// the same order, read from the library's code for gfx950 -- without the branches, selects and scalings that serve arguments
// outside the stated domain, so that on its domain it returns the library's result BIT FOR BIT
// (tests/test_gpu_fastmath_bits.py holds each to the library form on 2^22 random arguments and the domain's edges;
// tools/valu_budget.py counts the instructions of both forms).  A call site states why its argument lies inside the domain.
//
// Included from rng.h (inside namespace bssm, device compilation only).
#pragma once

// exp(x).  DOMAIN: x <= 0 (-inf included; a NaN comes back as NaN, as from the library).
// The library's exp: n = rint(x log2(e)), r = x - n ln2 (two-term), a degree-11 polynomial, ldexp by n, then two selects:
// +inf above 1024 and 0 below -1075.  On x <= 0 the first cannot fire and is dropped; the second stays -- it is what turns
// -inf (whose r is NaN) and arguments below the int range of n into 0; ldexp itself rounds the subnormal results.
__device__ __forceinline__ double exp_nonpos(double x)
{
    const double n = __builtin_rint(x * 0x1.71547652b82fep+0);
    double r = __builtin_fma(-0x1.62e42fefa39efp-1, n, x);
    r = __builtin_fma(-0x1.abc9e3b39803fp-56, n, r);
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
    const double z = __builtin_ldexp(p, (int)n);
    return (x < -1075.0) ? 0.0 : z;
}

// sqrt(x).  DOMAIN: x = +-0, or positive and normal with 2^-767 <= x < +inf.
// The library's sqrt: scale arguments below 2^-767 up by 2^256 (and the result back down), v_rsq_f64 and a fixed
// Goldschmidt / Newton sequence, then return x itself for +-0 and +inf.  Here: no scaling, and only the zero select.
__device__ __forceinline__ double sqrt_pos_normal(double x)
{
    const double y = __builtin_amdgcn_rsq(x);
    double g = x * y, h = y * 0.5;
    const double e = __builtin_fma(-h, g, 0.5);
    g = __builtin_fma(g, e, g);
    double d = __builtin_fma(-g, g, x);
    h = __builtin_fma(h, e, h);
    g = __builtin_fma(d, h, g);
    d = __builtin_fma(-g, g, x);
    g = __builtin_fma(d, h, g);
    return (x == 0.0) ? x : g;
}

// sin(pi x) and cos(pi x).  DOMAIN: 0 <= x <= 2.
// The library's sincospi: reduce |x| to r in [0, 2) (for |x| > 1: r = 2 fract(|x| / 2), which on (1, 2) is x itself and at 2 gives
// the same quadrant and remainder as r = 2), n = rint(2 r), f = r - n / 2 in [-1/4, 1/4], the two polynomials in f, quadrant
// selects on n, then the sign of x onto the sine and NaN for a non-finite x.  Here r = x, and the last two steps are dropped.
__device__ __forceinline__ void sincospi_0_2(double x, double* sn, double* cs)
{
    const double n = __builtin_rint(x + x);
    const double f = __builtin_fma(-0.5, n, x);
    const int i = (int)n;
    const double z = f * f;
    double p = __builtin_fma(z, 0x1.e357ef99eb0bbp-12, -0x1.e2fe76fdffd2bp-8);
    p = __builtin_fma(z, p, 0x1.50782d5f14825p-4);
    p = __builtin_fma(z, p, -0x1.32d2ccdfe9424p-1);
    p = __builtin_fma(z, p, 0x1.466bc67754fffp+1);
    p = __builtin_fma(z, p, -0x1.4abbce625be09p+2);
    const double fz = f * z;
    const double sp = __builtin_fma(0x1.921fb54442d18p+1, f, fz * p);
    double q = __builtin_fma(z, -0x1.b167302e21c33p-14, 0x1.f9c89ca1d4f33p-10);
    q = __builtin_fma(z, q, -0x1.a6d1e7294bff9p-6);
    q = __builtin_fma(z, q, 0x1.e1f5067b90b37p-3);
    q = __builtin_fma(z, q, -0x1.55d3c7e3c325bp+0);
    q = __builtin_fma(z, q, 0x1.03c1f081b5a67p+2);
    q = __builtin_fma(z, q, -0x1.3bd3cc9be45dep+2);
    const double cp = __builtin_fma(z, q, 1.0);
    const bool odd = i & 1;
    const unsigned long long flip = (unsigned long long)(unsigned)(i & 2) << 62;          // quadrants 2 and 3: both negated
    const double s = odd ? cp : sp, c = odd ? -sp : cp;
    *sn = __longlong_as_double((long long)((unsigned long long)__double_as_longlong(s) ^ flip));
    *cs = __longlong_as_double((long long)((unsigned long long)__double_as_longlong(c) ^ flip));
}

// ((double)(b >> 11) + 0.5) * 2^-53 for the 64 bits b = hi:lo.  DOMAIN: every b.
// The generic form shifts, converts the 53-bit quotient k in two halves, scales and adds them, adds 0.5 (which rounds once, when
// k >= 2^52) and scales: seven instructions.  Here k 2^11 = hi 2^32 + (lo with its low 11 bits cleared), exact in a double, needs no
// shift and one fma; adding 2^10 rounds (k + 0.5) 2^11 at the same place (a power-of-two scale commutes with the rounding: nothing
// here is subnormal), and the final scale by 2^-64 is exact -- six instructions, the same bits.
__device__ __forceinline__ double u01_from_bits_dev(uint32_t lo, uint32_t hi)
{
    const double h = (double)hi, l = (double)(lo & 0xFFFFF800u);
    const double t = __builtin_fma(h, 0x1.0p32, l);
    return __builtin_ldexp(t + 1024.0, -64);
}
