/* Host references for tests/test_gpu_device_math.py: the host libm (glibc) and __float128, elementwise over arrays.
   gcc -O2 -ffp-contract=off -shared -fPIC device_math_ref.c -o libdevice_math_ref.so -lm -lquadmath  (tests/device_prims.py: build_ref) */
#include <gnu/libc-version.h>
#include <math.h>
#include <quadmath.h>

const char *ref_libc_version(void) { return gnu_get_libc_version(); }

void ref_hypot(const double *x, const double *y, double *o, long n)
{
    for (long i = 0; i < n; i++) o[i] = hypot(x[i], y[i]);
}
void ref_atan2(const double *y, const double *x, double *o, long n)
{
    for (long i = 0; i < n; i++) o[i] = atan2(y[i], x[i]);
}
/* atan2 correctly rounded: __float128's atan2q (113 bits) rounded once to double */
void ref_atan2q(const double *y, const double *x, double *o, long n)
{
    for (long i = 0; i < n; i++) o[i] = (double)atan2q((__float128)y[i], (__float128)x[i]);
}
void ref_tanh(const double *x, double *o, long n)
{
    for (long i = 0; i < n; i++) o[i] = tanh(x[i]);
}
void ref_expm1(const double *x, double *o, long n)
{
    for (long i = 0; i < n; i++) o[i] = expm1(x[i]);
}
