// user_cost_ad.hpp -- second-order forward mode for the expansion of user-written cost functions (isls.costs.Custom).
//
// A user cost is a template `stage<S, P>(const S *x, const S *u, const P *par, int t, int N) -> S`.  The library compiles it at
// run time (hiprtc, gfx950) with S = T for the line search and the nominal cost, and with S = ad::Dual2<T> for the expansion:
// a hyper-dual number  v + a e1 + b e2 + ab e1 e2  (e1^2 = e2^2 = 0).  Seeded with the directions (e_i, e_j) of [x; u], one
// evaluation of stage() leaves  a = dc/dw_i,  b = dc/dw_j,  ab = d2c/dw_i dw_j  -- exact derivatives, no step size.  Four words
// per scalar whatever n + m is, so one lane carries one entry pair of the Hessian (user_cost.hpp spreads the pairs over lanes).
//
// The contract on S is that of user_model_ad.hpp, operation for operation: arithmetic and compound assignment with S or a plain
// number on either side, comparisons on the value part, sin cos sqrt exp log tanh asin atan2 fabs, isls::sin_cos, isls::py_mod,
// construction from a number.  sqrt at exactly 0 follows the first-order rule: a derivative part is 0 where the argument's parts
// that feed it are 0, and +-inf (not NaN) elsewhere.
#pragma once

#include "user_model_ad.hpp"

namespace isls {
namespace ad {

template <typename T>
struct Dual2 {
    using scalar = T;
    T v, a, b, ab;
    __host__ __device__ Dual2() : v(T(0)), a(T(0)), b(T(0)), ab(T(0)) {}
    __host__ __device__ Dual2(T x) : v(x), a(T(0)), b(T(0)), ab(T(0)) {}   // a constant
    __host__ __device__ Dual2(T x, T da, T db, T dab) : v(x), a(da), b(db), ab(dab) {}
    __host__ __device__ Dual2 &operator+=(const Dual2 &o) { return *this = *this + o; }
    __host__ __device__ Dual2 &operator-=(const Dual2 &o) { return *this = *this - o; }
    __host__ __device__ Dual2 &operator*=(const Dual2 &o) { return *this = *this * o; }
    __host__ __device__ Dual2 &operator/=(const Dual2 &o) { return *this = *this / o; }
};

// f(x) with f, f', f'' at x.v
template <typename T>
__device__ __forceinline__ Dual2<T> chain2(const Dual2<T> &x, T f, T fp, T fpp)
{
    return Dual2<T>(f, fp * x.a, fp * x.b, fp * x.ab + fpp * (x.a * x.b));
}

template <typename T>
__device__ __forceinline__ Dual2<T> operator+(const Dual2<T> &x) { return x; }
template <typename T>
__device__ __forceinline__ Dual2<T> operator-(const Dual2<T> &x) { return Dual2<T>(-x.v, -x.a, -x.b, -x.ab); }
template <typename T>
__device__ __forceinline__ Dual2<T> operator+(const Dual2<T> &x, const Dual2<T> &y)
{
    return Dual2<T>(x.v + y.v, x.a + y.a, x.b + y.b, x.ab + y.ab);
}
template <typename T>
__device__ __forceinline__ Dual2<T> operator-(const Dual2<T> &x, const Dual2<T> &y)
{
    return Dual2<T>(x.v - y.v, x.a - y.a, x.b - y.b, x.ab - y.ab);
}
template <typename T>
__device__ __forceinline__ Dual2<T> operator*(const Dual2<T> &x, const Dual2<T> &y)
{
    return Dual2<T>(x.v * y.v, x.a * y.v + x.v * y.a, x.b * y.v + x.v * y.b, (x.ab * y.v + x.v * y.ab) + (x.a * y.b + x.b * y.a));
}
template <typename T>
__device__ __forceinline__ Dual2<T> operator/(const Dual2<T> &x, const Dual2<T> &y)
{
    const T r = T(1) / y.v;
    return x * chain2(y, r, -r * r, T(2) * r * r * r);
}

#define ISLS_AD2_MIXED(OP)                                                                                                  \
    template <typename T>                                                                                                   \
    __device__ __forceinline__ Dual2<T> operator OP(const Dual2<T> &x, scalar_t<Dual2<T>> y) { return x OP Dual2<T>(y); }   \
    template <typename T>                                                                                                   \
    __device__ __forceinline__ Dual2<T> operator OP(scalar_t<Dual2<T>> x, const Dual2<T> &y) { return Dual2<T>(x) OP y; }
ISLS_AD2_MIXED(+)
ISLS_AD2_MIXED(-)
ISLS_AD2_MIXED(*)
ISLS_AD2_MIXED(/)
#undef ISLS_AD2_MIXED

#define ISLS_AD2_CMP(OP)                                                                                                    \
    template <typename T>                                                                                                   \
    __device__ __forceinline__ bool operator OP(const Dual2<T> &x, const Dual2<T> &y) { return x.v OP y.v; }                \
    template <typename T>                                                                                                   \
    __device__ __forceinline__ bool operator OP(const Dual2<T> &x, scalar_t<Dual2<T>> y) { return x.v OP y; }               \
    template <typename T>                                                                                                   \
    __device__ __forceinline__ bool operator OP(scalar_t<Dual2<T>> x, const Dual2<T> &y) { return x OP y.v; }
ISLS_AD2_CMP(<)
ISLS_AD2_CMP(<=)
ISLS_AD2_CMP(>)
ISLS_AD2_CMP(>=)
ISLS_AD2_CMP(==)
ISLS_AD2_CMP(!=)
#undef ISLS_AD2_CMP

template <typename T>
__device__ __forceinline__ Dual2<T> sin(const Dual2<T> &x)
{
    T s, c;
    sin_cos(x.v, s, c);
    return chain2(x, s, c, -s);
}
template <typename T>
__device__ __forceinline__ Dual2<T> cos(const Dual2<T> &x)
{
    T s, c;
    sin_cos(x.v, s, c);
    return chain2(x, c, -s, -c);
}
template <typename T>
__device__ __forceinline__ Dual2<T> sqrt(const Dual2<T> &x)
{
    const T rt = ::sqrt(x.v), fp = T(0.5) / rt, fpp = -fp / (T(2) * x.v);
    const T z = T(0);
    // 0, not 0 * inf, at x.v = 0 wherever the parts of the argument that feed a part of the result vanish (see the contract)
    return Dual2<T>(rt, x.a == z ? z : fp * x.a, x.b == z ? z : fp * x.b,
                    (x.ab == z ? z : fp * x.ab) + ((x.a == z || x.b == z) ? z : fpp * (x.a * x.b)));
}
template <typename T>
__device__ __forceinline__ Dual2<T> exp(const Dual2<T> &x)
{
    const T e = ::exp(x.v);
    return chain2(x, e, e, e);
}
template <typename T>
__device__ __forceinline__ Dual2<T> log(const Dual2<T> &x)
{
    const T r = T(1) / x.v;
    return chain2(x, ::log(x.v), r, -r * r);
}
template <typename T>
__device__ __forceinline__ Dual2<T> tanh(const Dual2<T> &x)
{
    const T t = ::tanh(x.v), d = T(1) - t * t;
    return chain2(x, t, d, T(-2) * t * d);
}
template <typename T>
__device__ __forceinline__ Dual2<T> asin(const Dual2<T> &x)
{
    const T q = T(1) - x.v * x.v, r = T(1) / ::sqrt(q);
    return chain2(x, ::asin(x.v), r, x.v * r / q);
}
template <typename T>
__device__ __forceinline__ Dual2<T> fabs(const Dual2<T> &x) { return chain2(x, ::fabs(x.v), x.v < T(0) ? T(-1) : T(1), T(0)); }
template <typename T>
__device__ __forceinline__ Dual2<T> atan2(const Dual2<T> &y, const Dual2<T> &x)
{
    const T q = T(1) / (x.v * x.v + y.v * y.v);
    const T gy = x.v * q, gx = -y.v * q;                       // gradient; Hessian: hyy = -hxx = -2 x y q^2, hxy = (y^2 - x^2) q^2
    const T hxx = T(2) * x.v * y.v * q * q, hxy = (y.v * y.v - x.v * x.v) * q * q;
    return Dual2<T>(::atan2(y.v, x.v), gy * y.a + gx * x.a, gy * y.b + gx * x.b,
                    (gy * y.ab + gx * x.ab) + hxx * (x.a * x.b - y.a * y.b) + hxy * (y.a * x.b + y.b * x.a));
}
template <typename T>
__device__ __forceinline__ Dual2<T> atan2(const Dual2<T> &y, scalar_t<Dual2<T>> x) { return atan2(y, Dual2<T>(x)); }
template <typename T>
__device__ __forceinline__ Dual2<T> atan2(scalar_t<Dual2<T>> y, const Dual2<T> &x) { return atan2(Dual2<T>(y), x); }

}  // namespace ad

template <typename T>
__device__ __forceinline__ void sin_cos(const ad::Dual2<T> &x, ad::Dual2<T> &s, ad::Dual2<T> &c)
{
    T sv, cv;
    sin_cos(x.v, sv, cv);
    s = ad::chain2(x, sv, cv, -sv);
    c = ad::chain2(x, cv, -sv, -cv);
}
// r = a - q b with the integer q of numpy's `%` (piecewise constant): every part is the same combination
template <typename T>
__device__ __forceinline__ ad::Dual2<T> py_mod(const ad::Dual2<T> &a, const ad::Dual2<T> &b)
{
    const T r = py_mod(a.v, b.v);
    const T q = rint((a.v - r) / b.v);
    return ad::Dual2<T>(r, a.a - q * b.a, a.b - q * b.b, (a.ab - q * b.ab));
}
template <typename T>
__device__ __forceinline__ ad::Dual2<T> py_mod(const ad::Dual2<T> &a, typename ad::Dual2<T>::scalar b)
{
    return py_mod(a, ad::Dual2<T>(b));
}
template <typename T>
__device__ __forceinline__ ad::Dual2<T> py_mod(typename ad::Dual2<T>::scalar a, const ad::Dual2<T> &b)
{
    return py_mod(ad::Dual2<T>(a), b);
}

}  // namespace isls
