// fe_atan and fe_tan: the arctangent and tangent of the fisheye lens model
// (DESIGN.md section 19), shared by the kernels of fisheye.hip and the host
// code (calib_solve.cpp, tests/cpp/fisheye_host_test.cpp) the way jpeg_pix.h is
// shared.
//
// libm's atan and tan differ between the device and glibc in the last place,
// and section 18 records why the project does not test through that.  So the
// contract is these two functions: each is a fixed sequence of f64 additions,
// multiplications and divisions (all correctly rounded, none contracted: the
// translation units that include this header are built with -ffp-contract=off),
// restated operation for operation in tests/fisheye_ref.py.
//
//   fe_atan(x), x >= 0 (NaN propagates; +inf gives pi/2): four break points
//       7/16, 11/16, 19/16, 39/16 move the argument to |t| < 7/16 by the
//       addition theorem against atan(0.5), atan(1), atan(1.5) and atan(inf),
//       each held as a high and a low word; then an odd minimax polynomial of
//       degree 23 in t, its even and odd halves summed apart.
//   fe_tan(t), t in [0, pi/2] (NaN propagates; any other t is evaluated by the
//       same operations and means nothing): t > pi/4 is mirrored to pi/2 - t
//       and the result inverted; an argument of 0.67434 or more is mirrored
//       once more to pi/4 - y, tan(y) = (1 - tan u) / (1 + tan u); what is left
//       is below 0.6744 and goes through an odd polynomial of degree 27.
//
// The polynomial coefficients are the minimax ones of the freely available
// fdlibm (atan: aT[0..10], tan: T[0..12]); the reductions here are this
// project's and simpler than fdlibm's, at the price of a few ulp (measured in
// DESIGN.md section 19).
#ifndef SLAMHIP_FISHEYE_MATH_H
#define SLAMHIP_FISHEYE_MATH_H

#if defined(__HIPCC__) || defined(__CUDACC__)
#define FE_FN __host__ __device__ inline
#else
#define FE_FN inline
#endif

namespace slamhip {

FE_FN double fe_atan(double x)
{
    // atan(0.5), atan(1), atan(1.5), atan(inf): high and low words
    const double hi0 = 4.63647609000806093515e-01, lo0 = 2.26987774529616870924e-17;
    const double hi1 = 7.85398163397448278999e-01, lo1 = 3.06161699786838301793e-17;
    const double hi2 = 9.82793723247329054082e-01, lo2 = 1.39033110312309984516e-17;
    const double hi3 = 1.57079632679489655800e+00, lo3 = 6.12323399573676603587e-17;
    double t, hi, lo;
    bool reduced = true;
    if (x < 0.4375) {
        t = x;
        hi = lo = 0;
        reduced = false;
    } else if (x < 0.6875) {
        t = (2.0 * x - 1.0) / (2.0 + x);
        hi = hi0;
        lo = lo0;
    } else if (x < 1.1875) {
        t = (x - 1.0) / (x + 1.0);
        hi = hi1;
        lo = lo1;
    } else if (x < 2.4375) {
        t = (x - 1.5) / (1.0 + 1.5 * x);
        hi = hi2;
        lo = lo2;
    } else {   // NaN lands here and stays NaN
        t = -1.0 / x;
        hi = hi3;
        lo = lo3;
    }
    const double z = t * t;
    const double w = z * z;
    const double s1 = z * (3.33333333333329318027e-01 +
                           w * (1.42857142725034663711e-01 +
                                w * (9.09088713343650656196e-02 +
                                     w * (6.66107313738753120669e-02 +
                                          w * (4.97687799461593236017e-02 + w * 1.62858201153657823623e-02)))));
    const double s2 = w * (-1.99999999998764832476e-01 +
                           w * (-1.11111104054623557880e-01 +
                                w * (-7.69187620504482999495e-02 +
                                     w * (-5.83357013379057348645e-02 + w * -3.65315727442169155270e-02))));
    const double p = t * (s1 + s2);
    if (!reduced) return t - p;
    return hi - ((p - lo) - t);
}

// the odd polynomial of fe_tan on |u| < 0.6744
FE_FN double fe_tan_poly(double u)
{
    const double z = u * u;
    const double w = z * z;
    const double r = 1.33333333333201242699e-01 +
                     w * (2.18694882948595424599e-02 +
                          w * (3.59207910759131235356e-03 +
                               w * (5.88041240820264096874e-04 +
                                    w * (7.81794442939557092300e-05 + w * -1.85586374855275456654e-05))));
    const double v = z * (5.39682539762260521377e-02 +
                          w * (8.86323982359930005737e-03 +
                               w * (1.45620945432529025516e-03 +
                                    w * (2.46463134818469906812e-04 +
                                         w * (7.14072491382608190305e-05 + w * 2.59073051863633712884e-05)))));
    const double s = z * u;
    return u + (z * (s * (r + v)) + 3.33333333333334091986e-01 * s);
}

FE_FN double fe_tan(double t)
{
    const double pio2_hi = 1.57079632679489655800e+00, pio2_lo = 6.12323399573676603587e-17;
    const double pio4_hi = 7.85398163397448278999e-01, pio4_lo = 3.06161699786838301793e-17;
    const bool big = t > pio4_hi;
    const double y = big ? (pio2_hi - t) + pio2_lo : t;
    const bool near = y >= 0.67434;
    const double u = near ? (pio4_hi - y) + pio4_lo : y;
    const double q = fe_tan_poly(u);
    const double ty = near ? (1.0 - q) / (1.0 + q) : q;
    return big ? 1.0 / ty : ty;
}

}  // namespace slamhip

#endif
