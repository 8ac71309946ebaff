// project_rows_body.inc -- body of the two row-projection kernels of project.hip, included once into each with `ROWS` a
// constexpr bool in scope (textual inclusion: the shared-operand kernel compiles exactly as it did before there was a second one).
// Names the including kernel must have in scope: its template parameters T (double / float) and D (row dimension), its
// argument ProjP<T> p, and `constexpr bool ROWS` (true: per-row tables, project_rows_moving_kernel); from projections.hpp:
// CSet, kMaxSets, kMaxSetDim, set_par_words and the four row algorithms; from isls_common.hpp: wave_max.  Nothing else is read.
    __shared__ T red[2][16];                                   // [a / b][wavefront]
    const int pb = blockIdx.x, r = threadIdx.x;
    if (p.active != nullptr && p.active[pb] == 0) return;      // uniform per workgroup
    const bool inr = r < p.R;
    const bool row = inr && (p.row_mask == nullptr || p.row_mask[inr ? r : 0] != 0);   // rows outside the mask pass through
    T x0[D], x[D];
    const T *src = p.y_in + (int64_t)pb * p.in_sp + (int64_t)(inr ? r : 0) * p.in_sr;
#pragma unroll
    for (int j = 0; j < D; ++j) x0[j] = src[j];
    CSet<T> sets[kMaxSets];
#pragma unroll
    for (int s = 0; s < kMaxSets; ++s) {
        sets[s].kind = p.kind[s];
        sets[s].dim = p.dim[s];
        sets[s].A = p.A[s] ? p.A[s] + (int64_t)pb * p.A_sp[s] : nullptr;
        sets[s].b = p.b[s] ? p.b[s] + (int64_t)pb * p.b_sp[s] : nullptr;
        sets[s].par = p.par[s] ? p.par[s] + (int64_t)pb * p.par_sp[s] : nullptr;
        if constexpr (ROWS) {
            // this row's block of the per-row tables; lanes beyond R read row 0's (as `src` above): a table of exactly R rows
            // ends where its allocation ends.  The block width of SQUARE / MULTILINEAR comes from row 0's q (all rows share it).
            const int rr = inr ? r : 0;
            sets[s].kind = p.kind[s] & ~ISLS_SET_ROW_FLAGS;
            if ((p.kind[s] & ISLS_SET_ROW_PAR) && sets[s].par)
                sets[s].par += (int64_t)rr * set_par_words(sets[s].kind, sets[s].dim, sets[s].par);
            if ((p.kind[s] & ISLS_SET_ROW_B) && sets[s].b) sets[s].b += (int64_t)rr * sets[s].dim;
        }
    }
    int it = 0;
    if (p.algorithm == ISLS_PROJ_ALG_ADMM && p.nsets == 1 && sets[0].A == nullptr) {   // direct primitive
        T v[kMaxSetDim];
#pragma unroll
        for (int i = 0; i < kMaxSetDim; ++i) v[i] = i < D ? x0[i < D ? i : 0] : T(0);
        project_primitive<T>(sets[0].kind, D, sets[0].par, v);
#pragma unroll
        for (int j = 0; j < D; ++j) x[j] = v[j];
    } else {
        const int nw = (blockDim.x + 63) >> 6, wid = r >> 6;
        // Workgroup-wide maxima once per inner iteration: two barriers per call (partials visible; buffer free again).  The set
        // operands stay in global memory here: staging them in LDS as sls_admm.hip does measured 7 % slower for config 4's rows
        // (151 vs 141 us: the fp64 kernel spills more).
        auto block_max = [&](T &a, T &b) {
            if (!row) { a = T(0); b = T(0); }
            a = wave_max(a);
            b = wave_max(b);
            if ((r & 63) == 0) { red[0][wid] = a; red[1][wid] = b; }
            __syncthreads();
            T ma = red[0][0], mb = red[1][0];
            for (int w = 1; w < nw; ++w) { ma = red[0][w] > ma ? red[0][w] : ma; mb = red[1][w] > mb ? red[1][w] : mb; }
            __syncthreads();
            a = ma;
            b = mb;
        };
        if (p.algorithm == ISLS_PROJ_ALG_DYKSTRA)
            it = dykstra_row<T, D>(x0, p.nsets, sets, p.max_iter, p.threshold, x, block_max);
        else if (p.algorithm == ISLS_PROJ_ALG_SOC)
            it = project_soc_row<T, D>(x0, sets[0], p.rho, p.max_iter, p.threshold, x, block_max);
        else
            it = project_set_convex_row<T, D>(x0, p.nsets, sets, p.rho, p.max_iter, p.threshold, x, block_max);
    }
    if (inr) {
        T *dst = p.y_out + (int64_t)pb * p.out_sp + (int64_t)r * p.out_sr;
#pragma unroll
        for (int j = 0; j < D; ++j) dst[j] = row ? x[j] : x0[j];
    }
    if (r == 0 && p.iters) p.iters[pb] = it;
