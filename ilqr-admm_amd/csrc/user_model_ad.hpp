// user_model_ad.hpp -- forward-mode dual numbers for the Jacobians of user-written forward models (isls.models.Custom).
//
// A user model is a template `step<S, P>(const S *x, const S *u, const P *par, S *xn)`.  The library compiles it at run time
// (hiprtc, gfx950) with S = T for the line search, the closed loops and Custom.__call__, and with S = ad::Dual<T, K> for the
// linearisation: A_t = dxn/dx and B_t = dxn/du come out of the derivative parts, so nobody writes get_AB.
//
// The contract -- what a model may use on S, and what this header provides for the dual type:
//   arithmetic     + - * / (unary and binary, with S or a plain number on either side), += -= *= /=
//   comparisons    < <= > >= == != (on the value part: branches follow the nominal, as autograd does)
//   functions      sin cos sqrt exp log tanh asin atan2 fabs, isls::sin_cos(a, s, c), isls::py_mod(a, b) (numpy's `%`)
//   construction   S(1.5), S(0): a constant (zero derivative)
// A plain number next to an S may be of any arithmetic type (`0.5 * x`, `isls::py_mod(x, 2)`, and for S = float
// `isls::py_mod(x[0], x[1] * x[1] + 1.0)`, whose second argument is a double): it is converted to the scalar type of S.
// sqrt at exactly 0: the derivative is 0 in every direction in which the argument's derivative is 0 (a constant, or a column of
// the Jacobian the argument does not depend on) and +-inf in the others -- not the NaN of 0 * inf, which would poison the whole
// Jacobian row.
// Anything else (other math functions, integer casts of S, inline assembly) is outside the contract: a source that uses it
// fails to compile for the dual type, and the compile error comes back to the caller with the log.
#pragma once

#include "isls_common.hpp"

namespace isls {
namespace ad {

template <typename T, int K>
struct Dual {
    using scalar = T;
    T v;
    T d[K];
    __host__ __device__ Dual() : v(T(0))
    {
#pragma unroll
        for (int k = 0; k < K; ++k) d[k] = T(0);
    }
    __host__ __device__ Dual(T x) : v(x)                       // a constant
    {
#pragma unroll
        for (int k = 0; k < K; ++k) d[k] = T(0);
    }
    __host__ __device__ Dual &operator+=(const Dual &b) { return *this = *this + b; }
    __host__ __device__ Dual &operator-=(const Dual &b) { return *this = *this - b; }
    __host__ __device__ Dual &operator*=(const Dual &b) { return *this = *this * b; }
    __host__ __device__ Dual &operator/=(const Dual &b) { return *this = *this / b; }
};

// the scalar operand of a mixed operation is a non-deduced context: `0.5 * x` works for Dual<float, K> too
template <typename D>
using scalar_t = typename D::scalar;

// v = f(a), d = fp * a.d
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> chain(const Dual<T, K> &a, T f, T fp)
{
    Dual<T, K> r;
    r.v = f;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = fp * a.d[k];
    return r;
}

template <typename T, int K>
__device__ __forceinline__ Dual<T, K> operator+(const Dual<T, K> &a) { return a; }
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> operator-(const Dual<T, K> &a) { return chain(a, -a.v, T(-1)); }

template <typename T, int K>
__device__ __forceinline__ Dual<T, K> operator+(const Dual<T, K> &a, const Dual<T, K> &b)
{
    Dual<T, K> r;
    r.v = a.v + b.v;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] + b.d[k];
    return r;
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> operator-(const Dual<T, K> &a, const Dual<T, K> &b)
{
    Dual<T, K> r;
    r.v = a.v - b.v;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] - b.d[k];
    return r;
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> operator*(const Dual<T, K> &a, const Dual<T, K> &b)
{
    Dual<T, K> r;
    r.v = a.v * b.v;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] * b.v + a.v * b.d[k];
    return r;
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> operator/(const Dual<T, K> &a, const Dual<T, K> &b)
{
    Dual<T, K> r;
    r.v = a.v / b.v;
    const T ib = T(1) / b.v;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = (a.d[k] - r.v * b.d[k]) * ib;
    return r;
}

#define ISLS_AD_MIXED(OP)                                                                                                    \
    template <typename T, int K>                                                                                             \
    __device__ __forceinline__ Dual<T, K> operator OP(const Dual<T, K> &a, scalar_t<Dual<T, K>> b) { return a OP Dual<T, K>(b); } \
    template <typename T, int K>                                                                                             \
    __device__ __forceinline__ Dual<T, K> operator OP(scalar_t<Dual<T, K>> a, const Dual<T, K> &b) { return Dual<T, K>(a) OP b; }
ISLS_AD_MIXED(+)
ISLS_AD_MIXED(-)
ISLS_AD_MIXED(*)
ISLS_AD_MIXED(/)
#undef ISLS_AD_MIXED

#define ISLS_AD_CMP(OP)                                                                                                      \
    template <typename T, int K>                                                                                             \
    __device__ __forceinline__ bool operator OP(const Dual<T, K> &a, const Dual<T, K> &b) { return a.v OP b.v; }             \
    template <typename T, int K>                                                                                             \
    __device__ __forceinline__ bool operator OP(const Dual<T, K> &a, scalar_t<Dual<T, K>> b) { return a.v OP b; }            \
    template <typename T, int K>                                                                                             \
    __device__ __forceinline__ bool operator OP(scalar_t<Dual<T, K>> a, const Dual<T, K> &b) { return a OP b.v; }
ISLS_AD_CMP(<)
ISLS_AD_CMP(<=)
ISLS_AD_CMP(>)
ISLS_AD_CMP(>=)
ISLS_AD_CMP(==)
ISLS_AD_CMP(!=)
#undef ISLS_AD_CMP

template <typename T, int K>
__device__ __forceinline__ Dual<T, K> sin(const Dual<T, K> &a)
{
    T s, c;
    sin_cos(a.v, s, c);
    return chain(a, s, c);
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> cos(const Dual<T, K> &a)
{
    T s, c;
    sin_cos(a.v, s, c);
    return chain(a, c, -s);
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> sqrt(const Dual<T, K> &a)
{
    const T rt = ::sqrt(a.v), fp = T(0.5) / rt;
    Dual<T, K> r;
    r.v = rt;
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] == T(0) ? T(0) : fp * a.d[k];   // 0, not 0 * inf, at a.v = 0 (see the contract)
    return r;
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> exp(const Dual<T, K> &a)
{
    const T e = ::exp(a.v);
    return chain(a, e, e);
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> log(const Dual<T, K> &a) { return chain(a, ::log(a.v), T(1) / a.v); }
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> tanh(const Dual<T, K> &a)
{
    const T t = ::tanh(a.v);
    return chain(a, t, T(1) - t * t);
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> asin(const Dual<T, K> &a) { return chain(a, ::asin(a.v), T(1) / ::sqrt(T(1) - a.v * a.v)); }
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> fabs(const Dual<T, K> &a) { return chain(a, ::fabs(a.v), a.v < T(0) ? T(-1) : T(1)); }
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> atan2(const Dual<T, K> &y, const Dual<T, K> &x)
{
    Dual<T, K> r;
    r.v = ::atan2(y.v, x.v);
    const T q = T(1) / (x.v * x.v + y.v * y.v);
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = (x.v * y.d[k] - y.v * x.d[k]) * q;
    return r;
}
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> atan2(const Dual<T, K> &y, scalar_t<Dual<T, K>> x) { return atan2(y, Dual<T, K>(x)); }
template <typename T, int K>
__device__ __forceinline__ Dual<T, K> atan2(scalar_t<Dual<T, K>> y, const Dual<T, K> &x) { return atan2(Dual<T, K>(y), x); }

}  // namespace ad

// the two helpers of the built-in models on dual numbers (isls_common.hpp has their T forms)
template <typename T, int K>
__device__ __forceinline__ void sin_cos(const ad::Dual<T, K> &a, ad::Dual<T, K> &s, ad::Dual<T, K> &c)
{
    T sv, cv;
    sin_cos(a.v, sv, cv);
    s = ad::chain(a, sv, cv);
    c = ad::chain(a, cv, -sv);
}
// r = a - q b with the integer q of numpy's `%`: dr = da - q db
template <typename T, int K>
__device__ __forceinline__ ad::Dual<T, K> py_mod(const ad::Dual<T, K> &a, const ad::Dual<T, K> &b)
{
    ad::Dual<T, K> r;
    r.v = py_mod(a.v, b.v);
    const T q = rint((a.v - r.v) / b.v);
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = a.d[k] - q * b.d[k];
    return r;
}
template <typename T, int K>
__device__ __forceinline__ ad::Dual<T, K> py_mod(const ad::Dual<T, K> &a, typename ad::Dual<T, K>::scalar b)
{
    return py_mod(a, ad::Dual<T, K>(b));
}
template <typename T, int K>
__device__ __forceinline__ ad::Dual<T, K> py_mod(typename ad::Dual<T, K>::scalar a, const ad::Dual<T, K> &b)
{
    return py_mod(ad::Dual<T, K>(a), b);
}
// S = T with a plain number of another arithmetic type on either side (for S = float, `x + 1.0` is a double, and py_mod(float,
// double) would be ambiguous between the two forms of isls_common.hpp): computed in float where one side is a float -- S is
// float then -- and in double otherwise, as the dual forms above compute in the scalar type of S
template <typename A, typename B,
          typename = std::enable_if_t<std::is_arithmetic<A>::value && std::is_arithmetic<B>::value && !std::is_same<A, B>::value &&
                                      (std::is_floating_point<A>::value || std::is_floating_point<B>::value)>>
__device__ __forceinline__ std::conditional_t<std::is_same<A, float>::value || std::is_same<B, float>::value, float, double>
py_mod(A a, B b)
{
    using R = std::conditional_t<std::is_same<A, float>::value || std::is_same<B, float>::value, float, double>;
    return py_mod(R(a), R(b));
}

}  // namespace isls
