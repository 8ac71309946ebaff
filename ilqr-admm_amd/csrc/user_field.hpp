// user_field.hpp -- a 2-D field for user-written costs (isls.costs.Custom(field=)): a signed-distance map, a terrain height
// map, a risk map, read inside `stage` and `constraint` as
//     isls::field(c, px, py)             c: a plain int channel; px, py: each an S or a plain number; the result is an S
// The field is C channels of nx x ny samples, sample [c, i, j] at (origin[0] + i spacing[0], origin[1] + j spacing[1]), shared by
// the batch.  The interpolant is the tensor-product cubic convolution with Keys' kernel at a = -1/2 (Catmull-Rom): C1, it
// interpolates the samples and reproduces polynomials up to degree 2 in each variable exactly.  Per axis, p = (pos - origin) /
// spacing:  pc = clamp(p, 0, n-1),  i = min(floor(pc), n-2),  s = pc - i,  taps i-1 .. i+2 with their indices clamped to
// [0, n-1] (FieldAxis: how the clamped taps are read), weights
//     w(-1) = (-s^3 + 2 s^2 - s) / 2    w(0) = (3 s^3 - 5 s^2 + 2) / 2    w(1) = (-3 s^3 + 4 s^2 + s) / 2    w(2) = (s^3 - s^2) / 2
// Where the clamp acts (p < 0 or p > n-1, decided on the value part as the contract's comparisons are) the derivative along that
// axis is zero: the field continues as a constant outside its grid.  A channel outside [0, C) is clamped.  A NaN position reads
// cell 0 (no index leaves the buffer) and gives NaN, value and derivatives: a diverged candidate of the line search stays one.
//
// The program text of a cost registered with a field (user_rtc.hip) defines ISLS_USER_COST_NFIELD = C and ISLS_USER_COST_FIELD_T
// = the program's precision and includes this header AHEAD of the user's source (a qualified name in a template is looked up
// where the template is written); a cost without a field never sees it, so isls::field does not exist there.  The descriptor
// below is the one variable of the module the host writes (hipModuleGetGlobal, whenever it loads a module of the cost): the
// samples themselves lie in one device buffer per precision that the registration owns, and isls_user_cost_set_field overwrites
// them in place.  It is __constant__: every read of it is a scalar load the compiler may hoist out of the step loop.
//
// The device side: 16 gathered read-only global loads per call -- four rows of four contiguous samples, one 32-bit offset from
// one base per row -- all issued before the first use (no branch around a load); one evaluation of the weight polynomials
// serves the value and every derivative; no LDS (the line search's launch plan stays the built-ins'), and no scratch of its
// own: every array below is indexed by unrolled constants.  Whether the KERNEL around it stays without scratch depends on the
// registers the stage needs on top of the roll-out's: the fp64 two-waves-per-SIMD variant is limited to 256, the roll-out alone
// takes about 235 of them there, one field read per step fits exactly, a stage with two chained reads spills (DESIGN.md 5k has
// the figures, tests/test_field_cost_host.py pins them).  On ad::Dual2 the second-order part is complete:
//     d2f = f_xx dx dx + 2 f_xy dx dy + f_yy dy dy + f_x d2x + f_y d2y
// with f_x .. f_yy from the derivative weights of the same 16 taps; the samples are plain T and never differentiated.
#pragma once

namespace isls {

template <typename T>
struct FieldDesc {
    const T *v;                    // [C, nx, ny]
    int n[2];                      // nx, ny
    // per axis: origin, 1 / spacing, n - 1, and the factors of the derivative weights 1 / (2 spacing), 1 / spacing^2 -- every
    // number `field` needs that does not depend on the position comes from here through scalar loads: one the kernel computed
    // itself from nx or 1 / spacing would be a loop invariant held in vector registers for the whole roll-out
    T org[2], inv[2], top[2], half_inv[2], inv2[2];
    void set(const T *values, int nx, int ny, const double *origin, const double *inv_spacing)
    {
        v = values; n[0] = nx; n[1] = ny;
        for (int a = 0; a < 2; ++a) {
            org[a] = (T)origin[a]; inv[a] = (T)inv_spacing[a]; top[a] = (T)(n[a] - 1);
            half_inv[a] = T(0.5) * inv[a]; inv2[a] = inv[a] * inv[a];
        }
    }
};

}  // namespace isls

#ifdef __HIPCC_RTC__
#include "user_cost_ad.hpp"

__constant__ isls::FieldDesc<ISLS_USER_COST_FIELD_T> isls_user_cost_field;

namespace isls {

// One axis: the window start j0 and the weights of orders 0 .. ORDER on the four CONTIGUOUS samples j0 .. j0 + 3.  The taps of
// cell i are i-1 .. i+2 with their indices clamped to [0, n-1]; in the first cell (i = 0) tap -1 falls on sample 0 and in the last
// (i = n-2) tap 2 on sample n-1, so there the window stays inside the grid, j0 = clamp(i-1, 0, n-4), and the weight of the clamped
// tap is added to its neighbour's -- the same sum, and one address per row of the window with the other three samples at
// constant offsets instead of sixteen clamped indices.  The derivative weights carry 1 / spacing and 1 / spacing^2 (0 where the
// position clamp acts): derivatives along the axis, not in grid units.
template <typename T, int ORDER>
struct FieldAxis {
    int j0;
    T w[4], d1[4], d2[4];
    // w = the weights of taps -1 .. 2, merged at the grid's edge
    static __device__ __forceinline__ void window(T (&w)[4], bool first, bool last)
    {
        const T a = w[0], b = w[1], c = w[2], d = w[3];
        w[0] = first ? a + b : (last ? T(0) : a);
        w[1] = first ? c : (last ? a : b);
        w[2] = first ? d : (last ? b : c);
        w[3] = first ? T(0) : (last ? c + d : d);
    }
    __device__ __forceinline__ FieldAxis(T pos, const FieldDesc<T> &D, int axis)
    {
        const int n = D.n[axis];
        const T p = (pos - D.org[axis]) * D.inv[axis], top = D.top[axis];
        const bool below = p < T(0), above = p > top, out = below || above;
        const T pc = below ? T(0) : (above ? top : p);         // the clamp; a NaN position fails both comparisons and stays NaN ...
        int i = (int)fmax(pc, T(0));                           // ... but reads cell 0 (fmax drops it): no index leaves the grid.  pc >= 0: the floor
        i = i > n - 2 ? n - 2 : i;
        const bool first = i == 0, last = i == n - 2;          // (n >= 4: never both)
        j0 = first ? 0 : (last ? n - 4 : i - 1);
        const T s = pc - T(i), s2 = s * s, h = T(0.5);         // (a NaN goes on into every weight: the result is NaN)
        w[0] = h * (s * (T(2) * s - s2 - T(1)));
        w[1] = h * (s2 * (T(3) * s - T(5)) + T(2));
        w[2] = h * (s * (T(4) * s - T(3) * s2 + T(1)));
        w[3] = h * (s2 * (s - T(1)));
        window(w, first, last);
        if constexpr (ORDER >= 1) {
            const T g = out ? T(0) : D.half_inv[axis];
            d1[0] = g * (T(4) * s - T(3) * s2 - T(1));
            d1[1] = g * (T(9) * s2 - T(10) * s);
            d1[2] = g * (T(8) * s - T(9) * s2 + T(1));
            d1[3] = g * (T(3) * s2 - T(2) * s);
            window(d1, first, last);
        }
        if constexpr (ORDER >= 2) {
            const T g = out ? T(0) : D.inv2[axis];
            d2[0] = g * (T(2) - T(3) * s);
            d2[1] = g * (T(9) * s - T(5));
            d2[2] = g * (T(4) - T(9) * s);
            d2[3] = g * (T(3) * s - T(1));
            window(d2, first, last);
        }
    }
};

// f[0] = value; ORDER >= 1: f[1] = f_x, f[2] = f_y; ORDER >= 2: f[3] = f_xx, f[4] = f_xy, f[5] = f_yy
template <typename T, int ORDER>
__device__ __forceinline__ void field_eval(int c, T px, T py, T (&f)[6])
{
    static_assert(sizeof(T) == sizeof(ISLS_USER_COST_FIELD_T), "isls::field: positions of the program's precision");
    const FieldDesc<T> &D = isls_user_cost_field;
    const int nx = D.n[0], ny = D.n[1];
    const FieldAxis<T, ORDER> ax(px, D, 0), ay(py, D, 1);
    c = c < 0 ? 0 : (c > ISLS_USER_COST_NFIELD - 1 ? ISLS_USER_COST_NFIELD - 1 : c);
    const T *const base = D.v;
    // C nx ny <= 2^24: every offset fits 32 bits.  0 <= j0 <= n - 4 on both axes: the window lies inside the grid
    const unsigned first = ((unsigned)c * (unsigned)nx + (unsigned)ax.j0) * (unsigned)ny + (unsigned)ay.j0;
    T s[4][4];
#pragma unroll
    for (int a = 0; a < 4; ++a)
#pragma unroll
        for (int b = 0; b < 4; ++b) s[a][b] = base[first + (unsigned)a * (unsigned)ny + (unsigned)b];
#pragma unroll
    for (int k = 0; k < 6; ++k) f[k] = T(0);
#pragma unroll
    for (int a = 0; a < 4; ++a) {
        // the row's sums along y of orders 0, 1, 2, then along x
        const T r0 = (ay.w[0] * s[a][0] + ay.w[1] * s[a][1]) + (ay.w[2] * s[a][2] + ay.w[3] * s[a][3]);
        f[0] += ax.w[a] * r0;
        if constexpr (ORDER >= 1) {
            const T r1 = (ay.d1[0] * s[a][0] + ay.d1[1] * s[a][1]) + (ay.d1[2] * s[a][2] + ay.d1[3] * s[a][3]);
            f[1] += ax.d1[a] * r0;
            f[2] += ax.w[a] * r1;
            if constexpr (ORDER >= 2) {
                const T r2 = (ay.d2[0] * s[a][0] + ay.d2[1] * s[a][1]) + (ay.d2[2] * s[a][2] + ay.d2[3] * s[a][3]);
                f[3] += ax.d2[a] * r0;
                f[4] += ax.d1[a] * r1;
                f[5] += ax.w[a] * r2;
            }
        }
    }
}

// ---- plain numbers: S = T, and a call whose positions are both literals -------------------------------------------------------
template <typename A, typename B, typename = std::enable_if_t<std::is_arithmetic<A>::value && std::is_arithmetic<B>::value>>
__device__ __forceinline__ ISLS_USER_COST_FIELD_T field(int c, A px, B py)
{
    using T = ISLS_USER_COST_FIELD_T;
    T f[6];
    field_eval<T, 0>(c, T(px), T(py), f);
    return f[0];
}

// ---- ad::Dual<T, K>: the gradient programs -------------------------------------------------------------------------------------
template <typename T, int K>
__device__ __forceinline__ ad::Dual<T, K> field(int c, const ad::Dual<T, K> &px, const ad::Dual<T, K> &py)
{
    T f[6];
    field_eval<T, 1>(c, px.v, py.v, f);
    ad::Dual<T, K> r;
    r.v = f[0];
#pragma unroll
    for (int k = 0; k < K; ++k) r.d[k] = f[1] * px.d[k] + f[2] * py.d[k];
    return r;
}
template <typename T, int K>
__device__ __forceinline__ ad::Dual<T, K> field(int c, const ad::Dual<T, K> &px, ad::scalar_t<ad::Dual<T, K>> py)
{
    return field(c, px, ad::Dual<T, K>(py));
}
template <typename T, int K>
__device__ __forceinline__ ad::Dual<T, K> field(int c, ad::scalar_t<ad::Dual<T, K>> px, const ad::Dual<T, K> &py)
{
    return field(c, ad::Dual<T, K>(px), py);
}

// ---- ad::Dual2<T>: the expansion ---------------------------------------------------------------------------------------------------
template <typename T>
__device__ __forceinline__ ad::Dual2<T> field(int c, const ad::Dual2<T> &px, const ad::Dual2<T> &py)
{
    T f[6];
    field_eval<T, 2>(c, px.v, py.v, f);
    return ad::Dual2<T>(f[0], f[1] * px.a + f[2] * py.a, f[1] * px.b + f[2] * py.b,
                        (f[1] * px.ab + f[2] * py.ab) + (f[3] * (px.a * px.b) + f[4] * (px.a * py.b + px.b * py.a) + f[5] * (py.a * py.b)));
}
template <typename T>
__device__ __forceinline__ ad::Dual2<T> field(int c, const ad::Dual2<T> &px, ad::scalar_t<ad::Dual2<T>> py)
{
    return field(c, px, ad::Dual2<T>(py));
}
template <typename T>
__device__ __forceinline__ ad::Dual2<T> field(int c, ad::scalar_t<ad::Dual2<T>> px, const ad::Dual2<T> &py)
{
    return field(c, ad::Dual2<T>(px), py);
}

}  // namespace isls
#endif  // __HIPCC_RTC__
