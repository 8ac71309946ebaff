/*
 * isls_hip.h -- C ABI of libisls_hip.so: the MI355X (gfx950) batched DP-form iLQR-ADMM hot path.
 *
 * The reference (chenjianxing1/iLQR-ADMM, package `isls`) is pure Python; it has NO FFI/plugin
 * boundary.  Its hot path is the set of Python functions cited next to every entry point below;
 * each entry point is the batched (B independent trajectories) device replacement of one of them.
 * `INTEGRATION.md` shows the ctypes stub a maintainer of the reference would add to bind them.
 *
 * Conventions
 *   - every pointer is a DEVICE pointer into caller-owned memory (torch tensors in our host code);
 *     the library allocates no device memory, keeps no global state (but the registry of user models,
 *     isls_user_model_create), and is re-entrant per stream
 *     (the one process-wide input: experiment switches read from the environment once -- ISLS_*_TPW trajectories per
 *     wavefront, ISLS_GAIN_FF=0 / ISLS_FF_V2=0 / ISLS_COL_ROWS=0 select the previous form of a kernel; results do not
 *     depend on them beyond rounding);
 *   - all launches are asynchronous on `stream` (a hipStream_t passed as void*; NULL = default stream);
 *   - return value: ISLS_OK or a negative ISLS_ERR_* (argument / unsupported-size / launch error);
 *     numerical trouble is reported per trajectory in the int32 `status[B]` bit mask instead;
 *   - dense arrays are C-contiguous row-major exactly like the reference's numpy arrays with a
 *     leading batch axis:  K[B,N,m,n], k[B,N,m], x[B,N,n], u[B,N,m] ...
 *   - `isls_view` = strided per-timestep operand: object (b,t) starts at p + b*sb + t*st (strides in
 *     ELEMENTS).  sb==0 shares it over the batch, st==0 over the horizon (LTI fast path);
 *   - `_f64` entry points read/write double, `_f32` float; struct scalars are always double;
 *   - `active` (nullable) : trajectories with active[b]==0 are skipped entirely (frozen: converged
 *     or failed, SURVEY section 5 "failure detection").
 *
 * (n,m) with fast (templated) kernels: {2,1} {4,2} {6,3} {9,3} (the reference notebooks' systems) and {3,1} {6,2} {2,2} {3,3} (with
 * them every get_double_integrator_AB(nb_dim <= 3, nb_deriv <= 3) system): isls_dims_supported(n, m).  Every other pair with
 * n <= 16, m <= 8 runs the generic kernels (isls_dims_generic); beyond that ISLS_ERR_UNSUPPORTED.  1 <= L <= 64.
 */
#ifndef ISLS_HIP_H
#define ISLS_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define ISLS_VERSION 107   /* 107: isls_gain_args.lin_on; 106: isls_ff_args.lin_on (model-structured feed-forward pass); 105: isls_outer_advance_*, isls_outer_args.begin_done; 104: isls_riccati_gain_ff_*; 103: project_rows: Dykstra / project_soc algorithms, shell + multilinear sets, row masks; 102: timing context, reduce table */

#define ISLS_OK 0
#define ISLS_ERR_ARG (-1)
#define ISLS_ERR_UNSUPPORTED (-2)
#define ISLS_ERR_LAUNCH (-3)
#define ISLS_ERR_COMPILE (-4)  /* isls_user_model_*: the run-time compile failed (log: isls_user_model_log) or hiprtc is absent */

/* status[b] bits */
#define ISLS_ST_NOT_PD 1     /* Quu not positive definite (reference: LinAlgError from dposv, isls/isls.py:296) */
#define ISLS_ST_NAN_COST 2   /* a line-search candidate produced a NaN cost (isls/isls.py:362) */
#define ISLS_ST_LS_REJECT 4  /* no candidate improved the cost (fp_success False, isls/isls.py:365-372) */
#define ISLS_ST_REG_MAX 8    /* isls_reg_update_*: the regularisation ladder ended (a raise would pass mu_max); the failure bit stays */

/* Quu solve: iLQR path uses Cholesky (isls/isls.py:296), SLS.solve_dp an explicit inverse (isls/sls.py:149-151) */
#define ISLS_SOLVE_CHOL 0
#define ISLS_SOLVE_INV 1

/* built-in forward models f(x,u) (reference: user callbacks in the notebooks) */
#define ISLS_MODEL_LTI 0    /* x+ = A x + B u ; par = [A(n*n), B(n*m)]            (isls/sls_base.py:49-53)       */
#define ISLS_MODEL_ARM3R 1  /* planar 3R arm, n=9 m=3 ; par = [dt]                 (3DoF notebooks cells 9-10)    */
#define ISLS_MODEL_CAR 2    /* car-simple, n=4 m=2 ; par = [dt]                    (Car notebooks cell 6)         */
#define ISLS_MODEL_DI 3     /* double integrator, n=2d m=d: the LTI model of get_double_integrator_AB(d, 2, dt)
                               (isls/utils.py:266-276) evaluated through its Kronecker structure
                               A=[[I,aI],[0,I]], B=[[b0 I],[b1 I]]: p+ = p + a v + b0 u, v+ = v + b1 u;
                               par = [a, b0, b1] = [A[0,d], B[0,0], B[d,0]]. Same values as ISLS_MODEL_LTI on
                               those matrices (the skipped terms are exact zeros), a sixth of the multiplies */

#define ISLS_MODEL_TASSA 4  /* Tassa car-parking model, n=4 m=2 ; par = [dt, d]      (notebooks/Tutorial.ipynb cell 8):
                               f = dt v, b = f cos w + d - sqrt(d^2 - (f sin w)^2), x+ = x + b cos th, y+ = y + b sin th,
                               th+ = th + asin(f sin w / d), v+ = v + a dt ; state [x,y,th,v], control [w,a]              */

/* User-written forward models (isls_user_model_create): ids >= ISLS_MODEL_USER_BASE name a registered user model.  The `model`
 * fields of isls_rollout_args, isls_linearize_args (also inside isls_advance_args), isls_dense_loop_args and of the blocks that
 * embed them take such an id like a built-in one; par = the model's n_par parameters ([n_par] shared, or per trajectory with
 * model_par_sb = n_par).  Fast (n, m) pairs only (isls_dims_supported), cost model ISLS_COST_VIA; no model hint (lin_on). */
#define ISLS_MODEL_USER_BASE 1024
#define ISLS_USER_MAX_PAR 16        /* parameters of a user model, at most                                             */
#define ISLS_USER_MAX_TAB 16        /* words per step of a user cost's or a user model's table, at most (isls_user_*_create_tab) */
#define ISLS_USER_MAX_FIELD 4       /* channels of a user cost's 2-D field, at most (isls_user_cost_create_field) */
#define ISLS_USER_MAX_FIELD_WORDS (1 << 24) /* samples of such a field over all its channels, at most */
#define ISLS_DTYPE_F64 0
#define ISLS_DTYPE_F32 1

/* cost models of the line search and of the cost expansion */
#define ISLS_COST_VIA 0     /* via-point quadratic (isls/sls_base.py:25-44): Qtab, ztab, seq, u_std                       */
#define ISLS_COST_PHUBER 1  /* control-quadratic + pseudo-Huber state cost (notebooks/Tutorial.ipynb cell 14):
                               sum_t [ sum_i cu_i u_ti^2 + sum_i cx_i ph(x_ti, px_i) ] + sum_i cf_i ph(x_{N-1,i}, pf_i),
                               ph(x,p) = sqrt(x^2 + p^2) - p ; cost_par = [cu(m), cx(n), px(n), cf(n), pf(n)]
                               (built into the kernels of ISLS_MODEL_TASSA; Qtab/ztab/seq/u_std are then ignored)         */

/* User-written costs (isls_user_cost_create): ids >= ISLS_COST_USER_BASE name a registered user cost.  The `cost_model` fields of
 * isls_rollout_args and isls_expand_args (and of the blocks that embed isls_rollout_args) take such an id like a built-in one, with
 * any built-in model of a fast (n, m) pair or a user model; cost_par = the cost's n_par parameters ([n_par] shared, or per
 * trajectory with cost_par_sb = n_par); Qtab / ztab / seq / u_std are then ignored.  isls_expand_quadratic_* serves such an id
 * for the gradients and the nominal cost only (Cxx == Cuu == NULL); the full expansion, with Cux, is isls_user_cost_expand_*.
 * isls_outer_advance_* refuses such an id in `exp` (ISLS_ERR_UNSUPPORTED): run it with exp.c0x == NULL and the user expansion
 * behind it on the same stream, with active = accept.outer_active.  No generic (n, m), no model hint (lin_on).
 * A cost registered with a per-step table of W words (isls_user_cost_create_tab: a reference to track, weights or an obstacle
 * that change along the horizon) takes the table in three of the fields it ignores otherwise, in isls_rollout_args and in
 * isls_expand_args alike, stateless like cost_par:
 *   ztab    = the table, [N, W] or [B, N, W] (row t: the W words `stage` gets as `row` at step t);
 *   ztab_sb = 0 (shared by the batch) or N * W (one table per trajectory);
 *   nvia    = W.
 * ISLS_ERR_ARG, before anything is launched: ztab == NULL, nvia != W, any other ztab_sb.  The values may change between two
 * launches (a receding-horizon window): nothing is compiled or bound for them. */
#define ISLS_COST_USER_BASE 1024

/* rollout flags */
#define ISLS_RO_NAN_TO_1E5 1   /* costs[isnan] = 1e5            (iterate_once_dp only, isls/isls.py:362)          */
#define ISLS_RO_ACCEPT_TEST 2  /* accept iff cost_best < cost_cur (isls/isls.py:365-369); else nominal is kept    */
#define ISLS_RO_ABSOLUTE 4     /* u = K x + k (xhat=uhat=0, alpha forced to 1): SLSBase.get_trajectory_dp         */

/* projections (z-step of ADMM) */
#define ISLS_PROJ_NONE 0
#define ISLS_PROJ_BOX 1        /* np.clip(x, lo, hi)   isls/projections.py:7-11 ; bounds per (t, dim), +-inf = free */
#define ISLS_PROJ_SETS 2       /* project_set_convex over the time steps, isls/projections.py:289-374 (isls_admm_args) */

typedef struct isls_view {
    const void *p;
    int64_t sb, st;
} isls_view;

/* ---------------------------------------------------------------------------------------------
 * Riccati backward pass, gain part.
 * Replaces iSLS.backward_pass_DP (isls/isls.py:229-308; K and the factors that do not depend on the
 * linear cost terms) and SLS.solve_dp(return_Qs=True) (isls/sls.py:85-166).
 *   V_{N-1} = Cxx[N-1];  for t = N-2..0:
 *     Qxx = Cxx + A'VA, Qux = Cux + B'VA, Quu = Cuu + B'VB
 *     K_t = -Quu^{-1} Qux   (Cholesky U'U, or explicit inverse in ISLS_SOLVE_INV mode)
 *     V   = Qxx + K'Quu K + Qux'K + K'Qux                         (no symmetrisation, isls.py:300-301)
 * Outputs (dense): K[B,N,m,n] (K[N-1]=0), Quu[B,N,m,m], Qux[B,N,m,n] and
 *   fac[B,N,m,m]: CHOL mode: upper factor U with the DIAGONAL STORED AS 1/U_ii (strict lower = 0);
 *                 INV  mode: Quu^{-1} (the reference's Quu_inv_log).
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_gain_args {
    int32_t B, N, n, m;
    int32_t solve_mode;
    int32_t _pad;
    isls_view A;    /* [.,.,n,n] */
    isls_view Bm;   /* [.,.,n,m] */
    isls_view Cxx;  /* [.,.,n,n] */
    isls_view Cuu;  /* [.,.,m,m] */
    isls_view Cux;  /* [.,.,m,n] ; p==NULL -> 0 */
    void *K, *Quu, *fac, *Qux; /* Quu, fac, Qux may all be NULL when `rec` is given (their consumers then read the records) */
    int32_t *status;       /* [B] OR-ed in */
    const int32_t *active; /* nullable */
    void *rec;             /* nullable: packed step records [A+B K | B | K | fac] (row-major blocks, RW = n*n+2*n*m+m*m words)
                            * for the feed-forward pass (isls_ff_args.rec).  Opaque to the caller: an allocation of
                            * isls_ff_record_elems(B,N,n,m) elements, laid out [ceil(B/T)][N][T][RW] with T = 64/(n+m)
                            * trajectories per wavefront, so that a wavefront streams one contiguous burst per step;
                            * steps t = N-1 are not written.  Scratch semantics: the places of trajectories that are
                            * inactive (or past the batch in the last wavefront) are overwritten too, with a copy of
                            * another trajectory's record -- a consumer must use the same `active` mask as this pass.
                            * SHARED layout (isls_ilqr_admm_outer_* only; the single-kernel entry points always write and read a
                            * record per trajectory): when the block declares the same inputs for every trajectory -- lin_on with
                            * ISLS_MODEL_DI and lin_par_sb == 0, Cxx.sb == 0, Cuu.sb == 0, Cux.p == NULL or Cux.sb == 0 -- and the
                            * driver's own feed-forward passes (ff.rec == rec, same hint, sequential: no segments) and line
                            * searches read these records, K_t and fac_t are the same for the whole batch and the driver keeps
                            * ONE set of lean records: written by the first wavefront alone (its T slots hold identical copies;
                            * the other wavefronts compute the same values and skip the record stores), read by every
                            * trajectory's feed-forward pass and line search from slot 0 of block 0.  Decided from these declared
                            * strides and hints, never from addresses or values.  K [B,N,m,n] is still written for every active
                            * trajectory; k, status and the `active` semantics are per trajectory as before.  After such a call
                            * the buffer holds nothing a pass outside the driver could read                                    */
    int32_t lin_on;        /* != 0 (rec given, Quu / fac / Qux NULL; else ISLS_ERR_UNSUPPORTED): A and Bm are what isls_linearize_*
                            * wrote for `lin_model`.  The records are then written LEAN -- [K | fac | model words] only, at their own
                            * dense stride in the same buffer -- for feed-forward passes with the same hint (isls_ff_args.lin_on); a
                            * reader without it would misread them (the entry points that see both blocks check this).
                            * ISLS_MODEL_DI: the pass also neither loads nor stages A, Bm and evaluates [A B]'V [A B] and A + B K
                            * from the two non-zero entries of every column -- the same sums in the same order: fp64 results
                            * bit-identical to the dense pass, fp32 equal to rounding.  ISLS_MODEL_ARM3R (n=9, m=3) and ISLS_MODEL_CAR (n=4, m=2): dense
                            * arithmetic, lean records with the model words behind fac.  Other models: ISLS_ERR_UNSUPPORTED */
    int32_t lin_model;
    const void *lin_par;   /* isls_linearize_args.model_par of that model */
    int64_t lin_par_sb;    /* its batch stride in words (0: shared) */
} isls_gain_args;

/* elements of the packed-record buffer (see isls_gain_args.rec) */
int64_t isls_ff_record_elems(int32_t B, int32_t N, int32_t n, int32_t m);

int isls_riccati_gain_f64(const isls_gain_args *a, void *stream);
int isls_riccati_gain_f32(const isls_gain_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Riccati backward pass, feed-forward part (once per ADMM iteration).
 * Replaces the v/k recursion of iSLS.backward_pass_DP (isls/isls.py:285-302) and SLS.solve_dp_ff
 * (isls/sls.py:168-202) with the cached K, Quu, fac, Qux of the gain pass:
 *   cx_t = c0x_t + 2 Qr_t (xhat_t - (zx_t - lx_t)),  cu_t = c0u_t + 2 Rr_t (uhat_t - (zu_t - lu_t))
 *   v_{N-1} = cx_{N-1};  for t = N-2..0:
 *     qx = cx + A'v, qu = cu + B'v, k_t = -Quu^{-1} qu, v = qx + K'qu + K'Quu k + Qux'k
 * (the ADMM regulariser of isls/sls.py:132-137 and of O2).  xhat/uhat NULL -> 0 (absolute
 * coordinates, SLS path).  Qr.p / Rr.p NULL -> that term (and zx,lx / zu,lu) is unused.
 * Output k[B,N,m] (k[N-1]=0).
 *
 * Time-parallel form (optional, `seg`).  The recursion is affine in v: v_t = Phi_t v_{t+1} + g_t and
 * k_t = Gamma_t v_{t+1} + h_t, where Phi_t, Gamma_t depend only on A, B and the gain-pass outputs.  With
 * the N-1 steps cut into nseg segments of seg_len steps, every segment recurses concurrently from
 * v_in = 0 (the last one from the terminal gradient), the true segment inputs follow from nseg-2 small
 * mat-vecs with the segment transfer matrices Psi_s = Phi_{t0} ... Phi_{t1-1}, and k_t += G_t v_in(seg(t))
 * with G_t = Gamma_t Phi_{t+1} ... Phi_{t1-1}.  G and Psi are produced once per gain pass by
 * isls_riccati_ff_prepare_* and reused by every ADMM iteration; the result equals the sequential
 * recursion up to rounding (a different association of the same sums).
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_ffseg {
    int32_t nseg;     /* <= 1 or G == NULL: sequential recursion over the whole horizon            */
    int32_t seg_len;  /* steps per segment; (nseg, seg_len) as returned by isls_ff_segments()       */
    void *G;          /* [B,N,m,n]     k_t correction operators          (prepare -> ff)           */
    void *Psi;        /* [B,nseg,n,n]  segment transfer matrices         (prepare -> ff)           */
    void *v;          /* [B,nseg,n]    scratch of the ff pass (segment-start values of v)          */
} isls_ffseg;

/* Effective segmentation of a horizon of N steps for a requested segment count: returns nseg (>= 1)
 * and stores the segment length; every segment is non-empty. */
int32_t isls_ff_segments(int32_t N, int32_t nseg_requested, int32_t *seg_len);

typedef struct isls_ff_args {
    int32_t B, N, n, m;
    int32_t solve_mode;
    int32_t _pad;                   /* ncol: 0 / 1 = one pass.  C > 1: the C feedback columns of isls_admm (isls/isls.py:578-590) in ONE
                                     * launch on the same records: zx, lx, zu, lu and k hold C blocks [C,B,N,.], seg.v holds [C,B,nseg,n],
                                     * c0x / c0u act on column 0 only (the other columns carry no cost gradient).  Record path with
                                     * time-invariant Qr / Rr only (else ISLS_ERR_UNSUPPORTED: call once per column) */
    isls_view A, Bm;
    isls_view c0x; /* [.,.,n] */
    isls_view c0u; /* [.,.,m] */
    isls_view Qr;  /* [.,.,n,n] nullable */
    isls_view Rr;  /* [.,.,m,m] nullable */
    const void *xhat, *uhat;        /* [B,N,n], [B,N,m] nullable */
    const void *zx, *lx, *zu, *lu;  /* ADMM consensus / scaled dual, dense */
    const void *K, *Quu, *fac, *Qux;
    void *k;
    const int32_t *active;
    isls_ffseg seg;                 /* zero-initialised => sequential */
    const void *rec;                /* nullable: the packed records the gain pass wrote (isls_gain_args.rec).  The pass then
                                     * reads them instead of A, Bm, K, Quu, fac, Qux and evaluates the same recursion as
                                     * v = cx + K'cu + (A + B K)'v, k = -Quu^-1 (cu + B'v): one contiguous 81-word burst per
                                     * step instead of 108 words in six streams (n=6, m=3); results equal up to rounding */
    const void *Qr_term;            /* nullable: the state weight block [n,n] of the LAST step (batch stride Qr.sb), replacing Qr
                                     * there -- a weight that is the same at every step but the terminal one (a terminal state
                                     * constraint: notebooks/3DoF robot/State and control bound constraints.ipynb cell 22) is
                                     * then passed with a zero time stride and keeps the one-hand-off record kernel.  Record
                                     * path with time-invariant Qr / Rr only (else ISLS_ERR_UNSUPPORTED: pass the full [N,n,n]) */
    int32_t lin_on;                 /* != 0 (record path only): A and Bm are what isls_linearize_* wrote for `lin_model`, and the gain pass
                                     * that wrote `rec` had the same hint (isls_gain_args.lin_on): the records are LEAN -- only the tail
                                     * [K | fac | model words] of every record, 28 instead of 82 words per step at n=6, m=3, 42 instead of
                                     * 150 at n=9 -- and the pass evaluates (A + B K)'v = A'v + K'(B'v) from the model's structure:
                                     * ISLS_MODEL_DI (A = [I aI; 0 I], B = [b0 I; b1 I]) or ISLS_MODEL_ARM3R (A = [I dtI 0; 0 I 0; J dtJ 0],
                                     * B = [hI; dtI; hJ], the six words of J = A[6:8,0:3] kept behind fac) or ISLS_MODEL_CAR (A = I + {a02, a12, a03, a13,
                                     * a23}, B = {b20, b31 = dt}: those six behind fac).  Only the one-hand-off form
                                     * reads them: time-varying Qr / Rr or a time-parallel `seg` are ISLS_ERR_UNSUPPORTED, another model
                                     * too.  The same products in another association: results equal up to rounding.  The caller must
                                     * NOT set it for A, Bm of its own (get_AB callbacks) */
    int32_t lin_model;
    const void *lin_par;            /* isls_linearize_args.model_par of that model */
    int64_t lin_par_sb;             /* batch stride of lin_par in words (0: shared) */
} isls_ff_args;

int isls_riccati_ff_f64(const isls_ff_args *a, void *stream);
int isls_riccati_ff_f32(const isls_ff_args *a, void *stream);

/* Gain pass and the first feed-forward pass in one launch: iSLS.backward_pass_DP computes K and k in the same backward
 * sweep (isls/isls.py:285-302); so does this entry, for the linear terms `ff` describes.  The outer driver uses it for the
 * first of its J feed-forward passes.  Conditions (else ISLS_ERR_UNSUPPORTED): g->rec != NULL and ff->rec == g->rec,
 * g->Quu == g->fac == g->Qux == NULL (records only), Qr / Rr absent or time-invariant (st == 0), same B, N, n, m,
 * solve_mode and active as `g`.  ff->seg is ignored (the sweep is sequential); outputs: everything `g` writes, and ff->k. */
int isls_riccati_gain_ff_f64(const isls_gain_args *g, const isls_ff_args *ff, void *stream);
int isls_riccati_gain_ff_f32(const isls_gain_args *g, const isls_ff_args *ff, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Regularised gain pass: exactly isls_riccati_gain_* (ff == NULL) or isls_riccati_gain_ff_* (ff != NULL: the first feed-forward
 * pass inside, ISLS_ERR_UNSUPPORTED where that entry is) run on Cuu_t + mu_b I for t <= N-2 -- and on Cxx_t + mu_b I for
 * t <= N-2 when on_x != 0; the terminal block Cxx_{N-1} is left alone.  mu_b >= 0 is per trajectory, so batch-shared Hessian
 * tables (zero batch stride) stay usable: the term is added inside the kernel.  This is the proximal term mu/2 |du|^2 (+ mu/2
 * |dx|^2) folded into the stage cost, so K, fac = chol(Quu), the records [A+BK | B | K | fac] and every pass that reads them keep
 * their meaning.  An all-zero mu gives the bits of the plain entry points -- with one exception of sign: the term enters as
 * C_ii + mu ahead of the sum, so a diagonal cost entry of -0.0 becomes +0.0, which shows (as +0.0 for -0.0) only where the
 * accumulated A'VA / B'VB term of that entry is -0.0 as well.
 * Forms: records + K (g->rec, Quu == fac == Qux == NULL) or the arrays (g->rec == NULL); both together, or g->lin_on, are
 * ISLS_ERR_UNSUPPORTED.  The generic (n, m) pairs take the array form.  status / active / record scratch semantics: isls_gain_args.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_reg_args {
    const void *mu;        /* [B], device, the pass's dtype */
    int32_t on_x;          /* != 0: Cxx_t + mu I as well */
    int32_t _pad;
} isls_reg_args;

int isls_riccati_gain_reg_f64(const isls_gain_args *g, const isls_ff_args *ff /* nullable */, const isls_reg_args *r, void *stream);
int isls_riccati_gain_reg_f32(const isls_gain_args *g, const isls_ff_args *ff /* nullable */, const isls_reg_args *r, void *stream);

/* The schedule of mu (iLQG.m's: Tassa, Erez, Todorov 2012), one flat kernel over the trajectories with active[b] != 0 (nullable:
 * all) that do not carry ISLS_ST_REG_MAX yet:
 *   raise: delta = max(factor, delta * factor), mu' = max(mu_min, mu * delta); if mu' > mu_max: status |= ISLS_ST_REG_MAX and mu,
 *          delta stay (the ladder ended: the failure bit stays too);
 *   lower: delta = min(1 / factor, delta / factor), mu = mu * delta if that is >= mu_min, else 0.
 * ISLS_REG_AFTER_GAIN: raise where status has ISLS_ST_NOT_PD, and where the raise succeeded clear that bit, set retry[b] = 1 and
 *   count one in *count (the caller zeroes it, reads it back and runs the gain pass again while it is non-zero -- with the mask of
 *   the first launch, or one that covers whole wavefronts: see the scratch semantics of isls_gain_args.rec); retry[b] = 0 elsewhere.
 * ISLS_REG_AFTER_LS: raise where status has ISLS_ST_LS_REJECT (the bit stays: the caller reads the verdict from it), lower where
 *   the step was accepted (neither ISLS_ST_LS_REJECT nor ISLS_ST_NOT_PD).  retry / count are not used.
 * mu, delta: [B] in the entry point's dtype; start a solve with delta = 1. */
#define ISLS_REG_AFTER_GAIN 0
#define ISLS_REG_AFTER_LS 1
typedef struct isls_reg_update_args {
    int32_t B, mode;
    int32_t *status;        /* [B] */
    const int32_t *active;  /* nullable */
    void *mu, *delta;       /* [B] */
    int32_t *retry;         /* [B], ISLS_REG_AFTER_GAIN (nullable) */
    int32_t *count;         /* [1], ISLS_REG_AFTER_GAIN (nullable) */
    double factor, mu_min, mu_max;
} isls_reg_update_args;

int isls_reg_update_f64(const isls_reg_update_args *a, void *stream);
int isls_reg_update_f32(const isls_reg_update_args *a, void *stream);

/* Operators of the time-parallel feed-forward pass (see isls_ffseg): run after the gain pass whenever
 * A, B, K, Quu, fac or Qux changed.  Writes seg.G for t < (nseg-1)*seg_len and seg.Psi for 1 <= s <= nseg-2. */
typedef struct isls_ff_prepare_args {
    int32_t B, N, n, m;
    int32_t solve_mode;
    int32_t _pad;
    isls_view A, Bm;
    const void *K, *Quu, *fac, *Qux;
    const int32_t *active;
    isls_ffseg seg;
    const void *rec;       /* nullable: the gain pass's packed records (isls_gain_args.rec); A .. Qux are then not read */
} isls_ff_prepare_args;

int isls_riccati_ff_prepare_f64(const isls_ff_prepare_args *a, void *stream);
int isls_riccati_ff_prepare_f32(const isls_ff_prepare_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Forward line-search rollout + cost + arg-min + winner trajectory.
 * Replaces iSLS.rollout_DP (isls/isls.py:310-334), the candidate costs / arg-min / acceptance of
 * iSLS.iterate_once_dp (isls.py:357-369), the quadratic via-point cost SLSBase.compute_cost
 * (isls/sls_base.py:25-44, no 1/2) and the augmented-Lagrangian terms of the ilqr_admm line search
 * (isls/isls.py:471-476, `(dx*dx)@Qr` precedence => weights are the ROW SUMS of Qr: wq, wr).
 *   candidate l: x_0 = xhat_0 ; u_t = K_t (x_t - xhat_t) + alpha_l k_t + uhat_t ; x_{t+1} = f(x_t,u_t)
 *   cost_l  = sum_t (x_t-z_t)'Q_t(x_t-z_t) + u_std |u_t|^2           (Q_t=Qtab[seq[t]], z_t=ztab[seq[t]])
 *   aug_l   = cost_l + sum_t wq_t.(x_t-(zx_t-lx_t))^2 + wr_t.(u_t-(zu_t-lu_t))^2
 *   best = first arg-min of aug ; x_out,u_out = trajectory of `best` ; cost_new = cost_best (plain)
 * Outputs: cost_all[B,L] (aug, nullable), best[B], cost_new[B], x_out[B,N,n], u_out[B,N,m].
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_rollout_args {
    int32_t B, N, n, m, L;
    int32_t model;
    int32_t flags;
    int32_t nvia;
    const void *model_par;
    int64_t model_par_sb;           /* 0 = shared */
    const void *K, *k, *xhat, *uhat;
    const void *x0;                 /* [B,n] nullable: default xhat[:,0] */
    const void *alphas;             /* [L] */
    const void *Qtab;               /* [.,nvia,n,n] */
    int64_t Qtab_sb;
    const void *ztab;               /* [.,nvia,n] */
    int64_t ztab_sb;
    const int32_t *seq;             /* [N] */
    const int32_t *q_nonzero;       /* [N] nullable hint: 0 where Q_t == 0 for every trajectory (term skipped) */
    double u_std;
    isls_view wq;                   /* [.,.,n] nullable */
    isls_view wr;                   /* [.,.,m] nullable */
    const void *zx, *lx, *zu, *lu;
    const void *cost_cur;           /* [B], ISLS_RO_ACCEPT_TEST only */
    void *cost_all;
    int32_t *best;
    void *cost_new;
    void *x_out, *u_out;
    int32_t *status;
    const int32_t *active;
    int32_t cost_model;             /* ISLS_COST_*, or the id of a user cost (>= ISLS_COST_USER_BASE) */
    int32_t cost_par_sb;            /* a user cost's parameters: 0 = shared, else n_par = one row per trajectory (built-in costs: 0) */
    const void *cost_par;           /* ISLS_COST_PHUBER: [m + 4n] shared by the batch; a user cost: [n_par] or [B, n_par] */
} isls_rollout_args;

int isls_rollout_ls_f64(const isls_rollout_args *a, void *stream);
int isls_rollout_ls_f32(const isls_rollout_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Row-wise projections onto an intersection of sets.
 * Replaces isls/projections.py: project_bound (7-11), project_soc_unit_batch (140-162),
 * project_square_batch (256-266, with the affine keep-out transform of the car notebook) and
 * project_set_convex (289-374): the inner ADMM
 *   x = (I + rho sum A_i'A_i)^-1 (x0 + rho sum A_i'(z_i - b_i - l_i)),  z_i = P_i(A_i x + b_i + l_i),
 *   l_i += A_i x + b_i - z_i
 * run for every row of a problem at once and stopped for all rows of that problem together (max-norm
 * residuals below `threshold`, or both relative changes below 1e-5), like one call of the reference.
 * P problems x R rows (<= 1024) of dimension d (<= ISLS_MAX_ROW_DIM); rows are addressed through
 * (sp, sr) element strides so that a coordinate block of a [B,N,n] state array can be projected in place.
 * nsets == 1 with sets[0].A == NULL applies the primitive directly (no iteration, dim == d).  `algorithm` selects
 * project_set_convex_dykstra or project_soc instead of project_set_convex; `row_mask` restricts a call to some rows.
 * ------------------------------------------------------------------------------------------- */
#define ISLS_MAX_ROW_DIM 4
#define ISLS_MAX_SET_DIM 5
#define ISLS_MAX_SETS 4
#define ISLS_SET_BOX 1       /* par: lo[dim], hi[dim]                                                  */
#define ISLS_SET_SOC_UNIT 2  /* (z, t) = first dim-1 entries, last entry; no parameters                */
#define ISLS_SET_SQUARE 3    /* par: q, l, u, c[q], W[q*q], Winv[q*q]: l <= ||W(y[:q]-c)||_inf <= u    */
#define ISLS_SET_LINEAR 4    /* par: l, u, a[dim]: l <= a'y <= u        (project_linear_batch, projections.py:30-43) */
#define ISLS_SET_QUADRATIC 5 /* par: l, u: l <= y'y/2 <= u              (project_quadratic_batch, projections.py:91-105) */
#define ISLS_SET_SHELL 6     /* par: l, u, c[dim]: l <= |y-c|^2/2 <= u, project_quadratic_batch(y - c, l, u) + c -- the spherical
                                keep-out shells of notebooks/Double integrator/...spherical obstacle avoidance.ipynb cell 12  */
#define ISLS_SET_MULTILINEAR 7 /* par: q, l[q], u[q], M[q*dim]: l <= M y <= u, y - M'(M M')^-1 (M y - clip(M y, l, u))
                                  (project_multilinear, projections.py:46-61); q <= ISLS_MAX_SET_DIM                           */
/* Moving sets: flag bits ORed into isls_cset.kind (isls_project_rows_* and what runs through it: isls_admm_update_*,
 * the outer driver, the column passes).  The rows of a problem are time steps there, and a flagged operand holds one block
 * per row, back to back, so that a keep-out region can move along the horizon:
 *   ISLS_SET_ROW_PAR  the block of row r of problem p starts at par + p*par_sp + r*Wp, Wp = words of the primitive's
 *                     parameter block as listed above (BOX 2 dim, SQUARE 3 + q + 2 q^2, LINEAR 2 + dim, QUADRATIC 2,
 *                     SHELL 2 + dim, MULTILINEAR 1 + 2 q + q dim).  For SQUARE and MULTILINEAR Wp is taken from row 0's q:
 *                     every row must carry the same q.  ISLS_ERR_ARG on ISLS_SET_SOC_UNIT, which has no parameters.
 *   ISLS_SET_ROW_B    b holds one [dim] offset per row, at b + p*b_sp + r*dim.  ISLS_PROJ_ALG_ADMM and ISLS_PROJ_ALG_SOC;
 *                     ISLS_ERR_ARG in the direct form and under ISLS_PROJ_ALG_DYKSTRA, where b is not used.
 * A stays per call or per problem.  par_sp == 0 / b_sp == 0: one table shared by all problems.  A table has at least R rows;
 * a caller that follows a longer table through time moves the pointer by whole rows between calls.  Additive within ABI
 * version 107: no struct changes, and a library built before the flags existed rejects a flagged kind with
 * ISLS_ERR_UNSUPPORTED (kind out of range) -- a loud failure, never a misread of the table as one block.
 * isls_sls_admm_* returns ISLS_ERR_UNSUPPORTED for a flagged set. */
#define ISLS_SET_ROW_PAR 0x100
#define ISLS_SET_ROW_B 0x200
#define ISLS_SET_ROW_FLAGS (ISLS_SET_ROW_PAR | ISLS_SET_ROW_B)

/* algorithm of isls_project_rows_* over the sets of a call */
#define ISLS_PROJ_ALG_ADMM 0     /* project_set_convex: consensus ADMM over A_i y + b_i in C_i   (projections.py:289-374)       */
#define ISLS_PROJ_ALG_DYKSTRA 1  /* project_set_convex_dykstra: alternating projections with corrections (projections.py:465-504);
                                    every set acts on the row itself (A, b unused, dim == d); threshold = tol on the summed
                                    squared correction change of a pass, at most max_iter + 1 passes                            */
#define ISLS_PROJ_ALG_SOC 2      /* project_soc: A y + b in the second-order cone by ADMM (projections.py:163-234); one set of
                                    kind ISLS_SET_SOC_UNIT with A [dim,d], b [dim]; threshold = tol                             */

typedef struct isls_cset {
    int32_t kind, dim;          /* primitive (ISLS_SET_*, | ISLS_SET_ROW_PAR / ISLS_SET_ROW_B) and dimension of A y + b */
    const void *A;              /* [dim, d] row-major; NULL only for the direct form                */
    const void *b;              /* [dim]; with ISLS_SET_ROW_B [rows, dim]                           */
    const void *par;            /* primitive parameters; with ISLS_SET_ROW_PAR [rows, Wp]           */
    int64_t A_sp, b_sp, par_sp; /* element strides between problems (0 = shared by all problems)    */
} isls_cset;

typedef struct isls_project_args {
    int32_t P, R, d, nsets;
    int32_t max_iter;
    int32_t algorithm;          /* ISLS_PROJ_ALG_* (0 = project_set_convex)                         */
    double rho, threshold;
    isls_cset sets[ISLS_MAX_SETS];
    const void *y_in;           /* rows y_in[p*in_sp + r*in_sr + 0..d)   */
    int64_t in_sp, in_sr;
    void *y_out;                /* may alias y_in                          */
    int64_t out_sp, out_sr;
    int32_t *iters;             /* [P] nullable: inner iterations run      */
    const int32_t *active;      /* [P] nullable                            */
    const int32_t *row_mask;    /* [R] nullable, shared by the problems: rows with row_mask[r] == 0 pass through unchanged and
                                 * take no part in the stop rule -- a constraint set that touches only some time steps (the
                                 * state-bounds notebook projects its last two rows, each with its own set: one call per set) */
    const struct isls_project_args *next;   /* nullable: a further stage applied in place to this stage's output (same P, R, rows,
                                 * active; its own sets / algorithm / row_mask): project_set_convex followed by Dykstra in the
                                 * obstacle notebook, or one stage per group of rows                                          */
} isls_project_args;

int isls_project_rows_f64(const isls_project_args *a, void *stream);
int isls_project_rows_f32(const isls_project_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * ADMM z/dual update with projection, residuals and the two stop rules.
 * Replaces the body of ADMM() after the x-step (isls/admm.py:43-85) with project_x/project_u given
 * as descriptors (box: isls/projections.py:7-11; ISLS_PROJ_SETS: project_set_convex, 289-374):
 *   z_prev = z ; z = Proj(relax*x + (1-relax)*z + lmb) ; r = x - z ; lmb += r
 *   prim = |r_x| + |r_u| ; dual = |z_x - z_prev_x| + |z_u - z_prev_u|        (unscaled 2-norms)
 *   stop  if prim<tol_abs and dual<tol_abs, else if both relative changes (vs res_prev, +1e-30) < tol_rel
 * res[B,2] receives (prim,dual); res_prev[B,2] is read then overwritten with them (init 1e6, admm.py:25-26);
 * active[b] is cleared when a stop rule fires (nullable => no stop rule evaluated); iters[b] counts the
 * executed ADMM iterations of trajectory b (the length of the reference's `logs`, admm.py:71).
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_admm_args {
    int32_t B, N, n, m;
    int32_t proj_x, proj_u;
    double relax, tol_abs, tol_rel;
    const void *xx, *xu;
    void *zx, *lx, *zu, *lu;   /* a NULL z pointer disables that block (project_x / project_u False) */
    isls_view x_lo, x_hi;      /* [.,.,n] */
    isls_view u_lo, u_hi;      /* [.,.,m] */
    void *res, *res_prev;
    int32_t *active;
    int32_t *iters;            /* [B] nullable: incremented for every trajectory updated by this call */
    /* ISLS_PROJ_SETS: the z block is project_set_convex (isls_project_rows) over the N rows (time steps) of
     * the coordinate block [col0, col0+d) of relax*x + (1-relax)*z + lmb, the other coordinates pass through
     * (the state constraint of notebooks/Car/Iterative LQR with state constraints.ipynb cell 18).  Of the
     * descriptor only d, nsets, sets, rho, max_iter, threshold are used. */
    const isls_project_args *x_sets, *u_sets;
    int32_t x_col0, u_col0;
    void *x_work, *u_work;     /* [B,N,n] / [B,N,m] caller-owned scratch (argument of the projection) */
} isls_admm_args;

int isls_admm_update_f64(const isls_admm_args *a, void *stream);
int isls_admm_update_f32(const isls_admm_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SLS-ADMM with chance constraints on the controls (config 5 of BASELINE.json).
 * Replaces the iteration of SLS.ADMM_SLS (isls/sls.py:319-454, project_u only) with project_u given as
 * set descriptors: project_set_convex (isls/projections.py:289-374) over the R = N*m rows
 * y = [d_u, phi_u] (dimension D = 1 + p) of one problem per call of the reference:
 *   x_u = Linv (r_side + rr .* (z - lmb)) ;  z = Proj(alpha x_u + (1-alpha) z + lmb) ;  lmb += x_u - z
 *   prim = |rr .* (x_u - z)|_F , dual = |rr .* (z - z_prev)|_F
 *   stop if both < tol, else if both relative changes (+1e-30) < rel_tol = 1e-2      (sls.py:417-430)
 * (once the primal residual has reached rounding level its relative change is noise, so the iteration at which
 * the second rule fires is not reproducible to the last step, in the reference either; rel_tol = 0 disables it)
 * z and lmb start at zero.  Linv [R,R] = (Su'Q Su + R + Rr)^-1 (symmetric) is shared by the P problems
 * (same dynamics and weights), r_side [P,R,D] = [Su'Q xd_p , -Su'Q Sx] and the constraint sets may differ
 * per problem.  rr [R] is the diagonal of Rr.  logs [P,max_iter,2] receives (prim, dual) per executed
 * iteration (rows beyond iters[p] are left untouched).
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_sls_admm_args {
    int32_t P, R, D, max_iter;
    double alpha, tol;
    double rel_tol;           /* relative-change stop rule; the reference hard-codes 1e-2 (sls.py:426)   */
    const void *Linv;
    const void *r_side;
    const void *rr;
    isls_project_args proj;   /* nsets, sets, rho, max_iter, threshold are used (d = D); a set with ISLS_SET_ROW_PAR /
                               * ISLS_SET_ROW_B is ISLS_ERR_UNSUPPORTED: the kernel stages one block per set in LDS, and its
                               * rows are not time steps */
    void *x_u;                /* [P,R,D] out: du = x_u[:,:,0], phi_u[:, :p] = x_u[:,:,1:]         */
    void *z, *lmb;            /* [P,R,D] out, nullable                                            */
    void *logs;               /* nullable                                                         */
    int32_t *iters;           /* [P] nullable                                                     */
} isls_sls_admm_args;

int isls_sls_admm_f64(const isls_sls_admm_args *a, void *stream);
int isls_sls_admm_f32(const isls_sls_admm_args *a, void *stream);

/* Closed loop of the dense causal SLS controller for M initial states (Monte-Carlo evaluation of the notebooks):
 *   u_i = k_i + sum_{j<=i} K[i, j] x_j ,  x_{i+1} = A x_i + B u_i          (isls/sls_base.py:91-105, noise_scale = 0)
 * A [n,n], B [n,m], K [N m, N n], k [N m], x0 [M,n] -> x_log [M,N,n], u_log [M,N,m]. */
int isls_sls_closed_loop_f64(int32_t M, int32_t N, int32_t n, int32_t m, const void *A, const void *B, const void *K,
                             const void *k, const void *x0, void *x_log, void *u_log, void *stream);
int isls_sls_closed_loop_f32(int32_t M, int32_t N, int32_t n, int32_t m, const void *A, const void *B, const void *K,
                             const void *k, const void *x0, void *x_log, void *u_log, void *stream);

/* ---------------------------------------------------------------------------------------------
 * SLS controller of a batch of problems: K = PHI_U Phi_x^-1, k = (I - K Su) du with Phi_x = Sw + Su PHI_U
 * (replaces SLS.controller, isls/sls.py:235-242), without the dense Sw, Su or an inverse.  For a causal (block lower
 * triangular) PHI_U, Phi_x is unit block lower triangular and
 *   X_s[s] = I , X_s[l+1] = A_l X_s[l] + B_l PHI_U[l, s]             (block column s of Phi_x, l = s .. N-2)
 *   K[t, s] = PHI_U[t, s] - sum_{l = s+1..t} K[t, l] X_s[l]           (s = t .. 0),   K[t, s] = 0 for s > t
 *   xd_0 = 0 , xd_{t+1} = A_t xd_t + B_t du_t ,  k_t = du_t - sum_{l <= t} K[t, l] xd_l
 * with the A_l, B_l of sls_dense.transfer_matrices_ltv (A_0 .. A_{N-2} are read).  Sums run in the order written, in the
 * entry point's precision.  A PHI_U with a non-zero entry above the block diagonal gets ISLS_CTL_NOT_CAUSAL in flags[b]; its
 * K, k are then NOT the controller (the caller takes the dense route for it).  1 <= n <= 16, 1 <= m <= 8, any N >= 1.
 * ------------------------------------------------------------------------------------------- */
#define ISLS_CTL_NOT_CAUSAL 1

typedef struct isls_sls_controller_args {
    int32_t B, N, n, m;
    isls_view A, Bm;        /* [.,.,n,n], [.,.,n,m]: a shared LTI pair (sb = st = 0) or a linearisation per problem            */
    const void *PHI_U;      /* [B, N m, N n] dense                                                                            */
    const void *du;         /* [B, N m]                                                                                       */
    void *K;                /* [B, N m, N n] out: every entry written, exact zeros above the block diagonal                   */
    void *k;                /* [B, N m] out                                                                                   */
    int32_t *flags;         /* [B] out: ISLS_CTL_NOT_CAUSAL or 0                                                              */
    void *work;             /* caller-owned scratch of isls_sls_controller_work_elems(B, N, n) elements (the blocks of Phi_x
                             * below its diagonal and xd); its size grows as B N^2 n^2 / 2, so large batches are cut into chunks */
} isls_sls_controller_args;

/* elements of the scratch buffer of isls_sls_controller_* (0 for invalid dimensions) */
int64_t isls_sls_controller_work_elems(int32_t B, int32_t N, int32_t n);

int isls_sls_controller_f64(const isls_sls_controller_args *a, void *stream);
int isls_sls_controller_f32(const isls_sls_controller_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Feedback columns of iSLS.isls_admm (isls/isls.py:503-712) in DP form.
 * The reference solves, per outer iteration, the dense normal equations
 *   [d_u, phi_u] = (Su'Q Su + R + Su'Qr Su + Rr)^-1 (r_side + Su'Qr x_reg + Rr u_reg)      (isls.py:571,580-588)
 *   [d_x, phi_x] = Su [d_u, phi_u] + [0, Sx]                                                (isls.py:589-590)
 * for the C = 1 + dim columns at once.  Column c is the minimiser of one time-varying LQ problem about the
 * nominal: column 0 with the cost gradients of the nominal and delta x_0 = 0, column j >= 1 with no cost
 * gradient and delta x_0 = e_j (first `dim` states), each with its own ADMM target (z - lmb)[c].  All columns
 * share the gains K_t of ONE Riccati gain pass (isls_riccati_gain_*); their feed-forward terms k[c] come from
 * C feed-forward passes (isls_riccati_ff_* with xhat = uhat = NULL and, for c >= 1, zero c0x / c0u), and this
 * entry point rolls them through the linearised dynamics:
 *   dx_0 = e_c ; du_t = K_t dx_t + k[c]_t ; dx_{t+1} = A_t dx_t + B_t du_t           (t < N-1)
 *   du_{N-1} = -Cuu_{N-1}^-1 ( [c == 0] c0u_{N-1} - 2 Rr_{N-1} (zu - lu)[c]_{N-1} )
 * The last control never acts on the state (SURVEY 8a quirk i): the dense form gives it the minimiser of its
 * own cost term, reproduced by the second line.  Arrays with a leading C are column-major: [C,B,N,.].
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_columns_args {
    int32_t B, N, n, m;
    int32_t C;              /* 1 + dim                                                            */
    int32_t _pad;
    isls_view A, Bm;        /* [.,.,n,n], [.,.,n,m]                                               */
    isls_view Cuu;          /* [.,.,m,m] control Hessian of the gain pass (2 R + 2 Rr)            */
    isls_view c0u;          /* [.,.,m]   control gradient at the nominal (2 R uhat)               */
    isls_view Rr;           /* [.,.,m,m] nullable (project_u False)                               */
    const void *K;          /* [B,N,m,n]                                                          */
    const void *k;          /* [C,B,N,m]                                                          */
    const void *zu, *lu;    /* [C,B,N,m] nullable with Rr                                         */
    void *dx, *du;          /* [C,B,N,n], [C,B,N,m] out                                           */
    const int32_t *active;  /* [B] nullable                                                       */
} isls_columns_args;

int isls_columns_rollout_f64(const isls_columns_args *a, void *stream);
int isls_columns_rollout_f32(const isls_columns_args *a, void *stream);

/* Monte-Carlo closed loop of a dense causal controller about a nominal through a built-in forward model
 * (iSLSBase.get_trajectory_sls, isls/isls_base.py:28-42, noise_scale = 0), M initial states:
 *   dx_j = x_j - xhat_j (j <= i) ; u_i = (K [dx_0 .. dx_i, 0 ..] + k)_i + uhat_i ; x_{i+1} = f(x_i, u_i)
 * K [N m, N n] (lower block triangular is not assumed, entries right of block i are not read), k [N m], the nominal
 * xhat [N,n] / uhat [N,m] of ONE problem (NULL = 0: absolute form), x0 [M,n] -> x_log [M,N,n], u_log [M,N,m]. */
typedef struct isls_dense_loop_args {
    int32_t M, N, n, m;
    int32_t model, _pad;
    const void *model_par;
    const void *K, *k;
    const void *xhat, *uhat;
    const void *x0;
    void *x_log, *u_log;
} isls_dense_loop_args;

int isls_dense_closed_loop_f64(const isls_dense_loop_args *a, void *stream);
int isls_dense_closed_loop_f32(const isls_dense_loop_args *a, void *stream);

/* z / dual step of isls_admm around the row projection (isls/isls.py:626-665), in two phases:
 *   phase 0:  z_prev <- z ;  work[b, t*d+i, c] <- relax x + (1-relax) z + lmb  (+ nom[b,t,i] for c == 0)
 *             ... project the rows of `work` (isls_project_rows_* on [B, N*d, C], or the caller's function) ...
 *   phase 1:  z <- work (- nom for c == 0) ; r = x - z ; lmb += r
 *             prim = |Qr r_x|_F + |Rr r_u|_F , dual = |Qr (z_x - z_prev_x)|_F + |Rr (z_u - z_prev_u)|_F
 *             stop if prim < tol_abs and dual < tol_abs, else if both relative changes (+1e-30) < tol_rel (1e-3)
 * `nom` is the nominal the notebooks add to the d column before projecting and remove afterwards
 * (notebooks/3DoF robot/State bounds and robust control bounds.ipynb cell 25); NULL when the caller's projection
 * does that itself.  A block with x == NULL is absent (project_x / project_u False).  res / res_prev / active /
 * iters as in isls_admm_args. */
typedef struct isls_columns_admm_args {
    int32_t B, N, n, m;
    int32_t C, phase;
    double relax, tol_abs, tol_rel;
    const void *xx, *xu;          /* [C,B,N,n], [C,B,N,m] x-step (nullable per block)             */
    void *zx, *lx, *zu, *lu;      /* [C,B,N,.]                                                    */
    void *zx_prev, *zu_prev;      /* [C,B,N,.] scratch between the phases                         */
    const void *x_nom, *u_nom;    /* [B,N,n], [B,N,m] nullable                                    */
    void *x_work, *u_work;        /* [B,N*n,C], [B,N*m,C] projection argument / result            */
    isls_view Qr, Rr;             /* residual weights, [.,.,n,n] / [.,.,m,m]                      */
    void *res, *res_prev;         /* [B,2]                                                        */
    int32_t *active;              /* [B] nullable                                                 */
    int32_t *iters;               /* [B] nullable                                                 */
} isls_columns_admm_args;

int isls_columns_admm_f64(const isls_columns_admm_args *a, void *stream);
int isls_columns_admm_f32(const isls_columns_admm_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One ADMM iteration of isls_admm (isls/isls.py:578-665) enqueued as a whole -- the feedback-column counterpart of
 * isls_ilqr_admm_outer_*:
 *   x-step   : the C feed-forward passes (`ff` in the column layout of ff._pad = C: one launch on the packed records where that
 *              form applies, else -- or when ff._pad == 1 asks for it -- one pass per column:
 *              the driver then offsets zx, lx, zu, lu, k per column and hands columns >= 1 the zero vectors zero_x / zero_u as
 *              cost gradients), then isls_columns_rollout (`cols`);
 *   line search on column 0 (`ls`, skipped when ls.L == 0: SLS.ADMM_SLS has none): isls_rollout_ls of u_nom + alpha d_u with
 *              zero gains (ls.K a zero array, ls.k = du[0]), then  du[0] <- alpha* du[0],  dx[0] <- x_out - xhat  for the active
 *              problems (isls.py:593-606);
 *   z-step   : isls_columns_admm phase 0, the row projections (proj_x / proj_u, nullable: block absent), phase 1 (`admm`;
 *              skipped when both blocks are absent: the unconstrained problem has no z-step);
 *   `log`    : nullable [B,2], receives admm.res behind the z-step;  `any_active`: see the field.
 * Nothing is exchanged with the host between the launches.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_columns_iteration_args {
    isls_ff_args ff;
    isls_columns_args cols;
    isls_rollout_args ls;
    isls_columns_admm_args admm;
    const isls_project_args *proj_x, *proj_u;
    const void *zero_x, *zero_u;    /* [n], [m] zeros (cost gradients of the columns >= 1 in the one-pass-per-column form) */
    void *log;
    int32_t *any_active;            /* nullable: one word, set to 1 when admm.active still holds a problem behind the z-step, else 0 --
                                     * the flag a host loop follows (copied to pinned memory, read when it has landed) instead of
                                     * reducing the mask itself */
} isls_columns_iteration_args;

int isls_columns_iteration_f64(const isls_columns_iteration_args *a, void *stream);
int isls_columns_iteration_f32(const isls_columns_iteration_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Quadratic via-point cost expansion about the nominal (the `Cts is None` branch of
 * backward_pass_DP, isls/isls.py:263-271, written out as arrays, plus the ADMM regulariser):
 *   Cxx[b,t] = 2 Q_t (+ 2 Qr_t) ; Cuu[b,t] = 2 u_std I (+ 2 Rr_t)
 *   c0x[b,t] = 2 Q_t (xhat_t - z_t) ; c0u[b,t] = 2 u_std uhat_t ; cost[b] = compute_cost(xhat,uhat)
 * Cxx/Cuu may be NULL (skip).  xhat/uhat NULL -> 0 (absolute coordinates).
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_expand_args {
    int32_t B, N, n, m;
    int32_t nvia, _pad;
    const void *Qtab; int64_t Qtab_sb;
    const void *ztab; int64_t ztab_sb;
    const int32_t *seq;
    double u_std;
    isls_view Qr, Rr;               /* nullable */
    const void *xhat, *uhat;
    void *Cxx, *Cuu;                /* [B,N,n,n], [B,N,m,m] nullable */
    void *c0x, *c0u;                /* [B,N,n], [B,N,m] */
    void *cost;                     /* [B] nullable */
    const int32_t *active;
    int32_t cost_model;             /* ISLS_COST_VIA: as above; ISLS_COST_PHUBER: gradient / (diagonal) Hessian of the
                                       pseudo-Huber cost about the nominal, the get_Cs callback of Tutorial.ipynb cell 16 */
    int32_t cost_par_sb;            /* as in isls_rollout_args */
    const void *cost_par;
    const int32_t *q_nonzero;       /* [N] nullable hint as in isls_rollout_args: 0 where Q_t == 0 for every trajectory */
} isls_expand_args;

int isls_expand_quadratic_f64(const isls_expand_args *a, void *stream);
int isls_expand_quadratic_f32(const isls_expand_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Linearisation of the built-in models along the nominal: the user's get_AB(xhat,uhat) callback
 * (isls/isls.py:61-66,95; notebooks).  A[B,N,n,n], B[B,N,n,m] dense outputs.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_linearize_args {
    int32_t B, N, n, m;
    int32_t model, _pad;
    const void *model_par; int64_t model_par_sb;
    const void *xhat, *uhat;
    void *A, *Bm;
    const int32_t *active;
} isls_linearize_args;

int isls_linearize_f64(const isls_linearize_args *a, void *stream);
int isls_linearize_f32(const isls_linearize_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * End of an outer iteration: nominal_values <- last x-step of the ADMM (isls/isls.py:488; the setter
 * isls/isls_base.py:80-85 appends the new cost to cost_log) followed by the two outer stop rules
 * (isls/isls.py:493-499), per trajectory, for the trajectories with outer_active[b] != 0:
 *   xhat <- xx, uhat <- xu, prev = cost, cost <- cost_new, cost_hist <- push(cost)
 *   stop if |cost - prev| < tol_cost, or |mean(hist[-4:]) - mean(hist[-8:-4])| < tol_osc (needs >= 5 entries)
 * cost_hist[B,8] holds the tail of cost_log (oldest first), hist_len[B] its fill (<= 8).  A negative
 * tolerance disables that rule.  Stopped trajectories get outer_active[b] <- 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_accept_args {
    int32_t B, N, n, m;
    const void *xx, *xu, *cost_new;
    void *xhat, *uhat, *cost;
    void *cost_hist;        /* nullable (then the oscillation rule is skipped) */
    int32_t *hist_len;
    double tol_cost, tol_osc;
    int32_t *outer_active;  /* nullable => every trajectory is updated, no stop rule */
} isls_accept_args;

int isls_accept_step_f64(const isls_accept_args *a, void *stream);
int isls_accept_step_f32(const isls_accept_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Convergence reduction over the local batch shard: out[5] = { sum cost, max prim, max dual,
 * #active, #status!=0 } -- the 40-byte payload of the per-iteration RCCL all-reduce.
 * Batched analogue of the scalar tests at isls/isls.py:125-132,493-499 and isls/admm.py:72-85.
 * ------------------------------------------------------------------------------------------- */
int isls_reduce_convergence_f64(int32_t B, const void *cost, const void *res, const int32_t *active,
                                const int32_t *status, void *out5, void *stream);
int isls_reduce_convergence_f32(int32_t B, const void *cost, const void *res, const int32_t *active,
                                const int32_t *status, void *out5, void *stream);
/* The same reduction written straight into the [W,5] table of the all-reduce: row `rank` receives the five numbers, the
 * other W-1 rows are zeroed (so that one sum-all-reduce of the table gathers every rank's row; isls/shard.py). */
int isls_reduce_convergence_table_f64(int32_t B, const void *cost, const void *res, const int32_t *active,
                                      const int32_t *status, void *table, int32_t rank, int32_t world, void *stream);
int isls_reduce_convergence_table_f32(int32_t B, const void *cost, const void *res, const int32_t *active,
                                      const int32_t *status, void *table, int32_t rank, int32_t world, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One outer DP-form iLQR-ADMM iteration enqueued as a whole (SURVEY 3.3 with the dense solve
 * replaced by the Riccati pass): gain -> J x [ ff -> rollout/line-search -> ADMM update ].
 * The sub-structs are used as given; between inner iterations nothing is exchanged with the host.
 * `log` (nullable) receives res per inner iteration: log[j,B,2].  Before the first inner iteration,
 * for the trajectories with outer_active[b]!=0 (nullable => all): admm.active[b] <- 1, lambda <- 0
 * (isls/isls.py:414-415,482), res_prev <- 1e6 (isls/admm.py:25-26); the others get admm.active[b] <- 0.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_outer_args {
    isls_gain_args gain;
    isls_ff_args ff;
    isls_rollout_args ro;
    isls_admm_args admm;
    int32_t J;
    int32_t skip_gain;          /* reuse the cached factors (is_dynamics_linear && is_cost_quadratic);
                                 * when the gain pass runs and ff.seg is set, the ff operators are prepared too */
    int32_t begin_done;         /* 1: the start-of-iteration resets described above have been made already (by
                                 * isls_outer_advance_* at the end of the previous iteration) and are skipped here */
    int32_t _pad;
    void *log;
    const int32_t *outer_active;
    void *timing;               /* nullable: isls_timing_create() context that records the kernel-family durations */
} isls_outer_args;

int isls_ilqr_admm_outer_f64(const isls_outer_args *a, void *stream);
int isls_ilqr_admm_outer_f32(const isls_outer_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * End of one outer iteration and start of the next in ONE launch: what the reference does between two x-step solves
 * (isls/isls.py:488-499, then 61-66 / 95-102 / 414-415 of the next pass through the loop), per trajectory:
 *   1. `accept`  : isls_accept_step_* semantics (nominal <- x-step, cost log, the two stop rules -> outer_active);
 *   2. for the trajectories still iterating afterwards: admm_active <- 1, lambda <- 0, res_prev <- 1e6, iters <- 0 (the others:
 *      admm_active <- 0) -- the resets isls_ilqr_admm_outer_* starts with (pass begin_done = 1 there);
 *   3. `lin`     : isls_linearize_* about the new nominal   (lin.A == NULL: skipped; lin.active is ignored; a user model's
 *                  linearisation is a second launch on the same stream, behind the first);
 *   4. `exp`     : isls_expand_quadratic_* about it         (exp.c0x == NULL: skipped; exp.active is ignored).
 * Same results as the four calls in that order with active = accept.outer_active.  lin / exp normally name accept.xhat /
 * accept.uhat as their nominal.  admm_active, lx, lu, res_prev, iters are nullable.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_advance_args {
    isls_accept_args accept;
    isls_linearize_args lin;
    isls_expand_args exp;
    int32_t *admm_active;       /* [B] */
    int32_t *iters;             /* [B] */
    void *lx, *lu;              /* [B,N,n], [B,N,m] scaled duals of the ADMM */
    void *res_prev;             /* [B,2] */
} isls_advance_args;

int isls_outer_advance_f64(const isls_advance_args *a, void *stream);
int isls_outer_advance_f32(const isls_advance_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * User-written forward models, compiled at run time for gfx950 (hiprtc, dlopen-ed on the first create; nothing else in the
 * library depends on it).  `source` defines
 *     template <typename S, typename P> __device__ void step(const S *x, const S *u, const P *par, S *xn);
 * in plain arithmetic on S (the contract: csrc/user_model_ad.hpp); no inline assembly, no __builtin_amdgcn_*.  It is
 * compiled with S = T for the line search (the built-ins' rollout kernel template and launch plans), the closed loop and
 * isls_user_model_step, and with S = a forward-mode dual number for isls_linearize_* (A_t, B_t without a get_AB).  The
 * headers are read from the directory of libisls_hip.so.  The library keeps the registry of user models (process-wide, for
 * the life of the process); it is the one piece of state it holds.
 * ------------------------------------------------------------------------------------------- */
/* Compiles `source` (fp64 now, fp32 on first use) and registers it: *id >= ISLS_MODEL_USER_BASE, also when the compile
 * fails (ISLS_ERR_COMPILE; its log stays readable).  ISLS_ERR_UNSUPPORTED: (n, m) not a fast pair, n_par outside
 * [0, ISLS_USER_MAX_PAR]; ISLS_ERR_ARG: a source with `asm` or `__builtin_amdgcn`.  Needs no GPU. */
int isls_user_model_create(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t *id);
/* The compile log (NUL-terminated, truncated to len - 1 characters); returns its full length, or a negative ISLS_ERR_*. */
int64_t isls_user_model_log(int32_t id, char *buf, int64_t len);
/* The gfx950 code object of the model for dtype (ISLS_DTYPE_*): *len <- its size; copied to buf when buf != NULL and *len
 * (on input) is large enough.  Compiles the dtype if it has not been yet. */
int isls_user_model_code(int32_t id, int32_t dtype, void *buf, int64_t *len);
/* Loads the model's module for dtype onto the current device (once; call it outside any stream capture). */
int isls_user_model_load(int32_t id, int32_t dtype);
/* xn[r] = f(x[r], u[r]) for R rows: x [R,n], u [R,m], par [n_par] (par_sb = 0) or [R,n_par] (par_sb = n_par) -> xn [R,n]. */
int isls_user_model_step_f64(int32_t id, int32_t R, const void *par, int64_t par_sb, const void *x, const void *u, void *xn,
                             void *stream);
int isls_user_model_step_f32(int32_t id, int32_t R, const void *par, int64_t par_sb, const void *x, const void *u, void *xn,
                             void *stream);

/* A model with a per-step table of n_tab words (1 .. ISLS_USER_MAX_TAB): a schedule, a forecast, a variable time step, a linear
 * time-varying system.  `source` then defines the five-argument form
 *     template <typename S, typename P> __device__ void step(const S *x, const S *u, const P *par, const P *row, S *xn);
 * `row` the n_tab words of step t (plain P: nothing is differentiated with respect to them); a source of the other form is a
 * compile error.  The table travels stateless, behind the parameters in the buffer every argument block names as the model's
 * (model_par / par), per trajectory or once for the batch:
 *     [ par (n_par) | row 0 | row 1 | ... | row N-1 ],     batch stride 0 or n_par + N * n_tab.
 * ISLS_ERR_ARG, before anything is compiled for a pair, loaded or launched: model_par == NULL, any other stride.  The values may
 * change between two launches (a receding-horizon window): nothing is compiled or bound for them.
 * Served: isls_rollout_ls_* (and the drivers that embed it: the row of a step arrives with the step's other operands, prefetched
 * into a side record in LDS), isls_linearize_* (also inside isls_outer_advance_*), isls_sample_nominal_* / _fb_*, isls_mpc_step_*
 * (the re-roll reads row t of model_par as it stands at the launch; the plant steps with row 0 of plant_par, the same layout,
 * which need not reach further than that row: plant_sb == 0 or >= n_par + n_tab) and isls_user_model_step_tab_*.
 * Not served, ISLS_ERR_UNSUPPORTED: isls_dense_closed_loop_*, isls_mc_closed_loop_* (fold the schedule into the state, or run the
 * loop step by step).  ISLS_ERR_UNSUPPORTED from the create: n_tab outside [0, ISLS_USER_MAX_TAB]. */
int isls_user_model_create_tab(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t *id);
/* Words per step of the model's table (0: a model without one); ISLS_ERR_ARG: no such model. */
int isls_user_model_n_tab(int32_t id);
/* isls_user_model_step for a table model: the R state rows come in runs of `run` rows per parameter block (par: [par | N rows],
 * par_sb = 0 or n_par + N * n_tab per run); row r steps with table row t[r] (t: R device words in [0, N)), or, t == NULL, with its
 * place r % run in its run (run <= N).  A table model steps through this entry only, and only a table model does. */
int isls_user_model_step_tab_f64(int32_t id, int32_t R, int32_t run, int32_t N, const void *par, int64_t par_sb, const int32_t *t,
                                 const void *x, const void *u, void *xn, void *stream);
int isls_user_model_step_tab_f32(int32_t id, int32_t R, int32_t run, int32_t N, const void *par, int64_t par_sb, const int32_t *t,
                                 const void *x, const void *u, void *xn, void *stream);

/* ---------------------------------------------------------------------------------------------
 * User-written cost functions, compiled at run time for gfx950 like the user models.  `source` defines
 *     template <typename S, typename P> __device__ S stage(const S *x, const S *u, const P *par, int t, int N);
 * the cost of step t; the total cost is sum_{t=0}^{N-1} stage(x_t, u_t, par, t, N) (a terminal term: `if (t == N - 1)`; u_{N-1}
 * is costed).  Plain arithmetic on S (the contract: csrc/user_model_ad.hpp); no inline assembly, no __builtin_amdgcn_*.  It is
 * compiled with S = T into the rollout kernel of the built-in models (the line search; one program per model it is used with)
 * and the row-wise value, and with S = a hyper-dual number (csrc/user_cost_ad.hpp) for the expansion: gradient and full
 * Hessian, Cux included, without a get_Cs.  The registry of user costs is process-wide, for the life of the process.
 * ------------------------------------------------------------------------------------------- */
/* Compiles `source` (fp64: the expansion and the value) and registers it: *id >= ISLS_COST_USER_BASE, also when the compile fails
 * (ISLS_ERR_COMPILE; its log stays readable).  ISLS_ERR_UNSUPPORTED: (n, m) not a fast pair, n_par outside
 * [0, ISLS_USER_MAX_PAR]; ISLS_ERR_ARG: a source with `asm` or `__builtin_amdgcn`.  Needs no GPU. */
int isls_user_cost_create(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t *id);
/* The same for a cost with a per-step table of n_tab words: `source` then defines the six-argument form
 *   template <typename S, typename P> __device__ S stage(const S *x, const S *u, const P *par, const P *row, int t, int N);
 * (`row`: the n_tab words of step t, plain P).  n_tab = 0 is isls_user_cost_create; a source of the other form than n_tab says is
 * a compile error.  ISLS_ERR_UNSUPPORTED: n_tab outside [0, ISLS_USER_MAX_TAB]. */
int isls_user_cost_create_tab(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t *id);
/* Words per step of the cost's table (0: a cost without one), or ISLS_ERR_ARG for an id nobody registered. */
int isls_user_cost_n_tab(int32_t id);
/* Nonlinear path constraints g(x, u) <= 0 by augmented Lagrangian.  A cost registered with n_con = K >= 1 constraints defines,
 * next to `stage`,
 *   template <typename S, typename P> __device__ void constraint(const S *x, const S *u, const P *par, int t, int N, S *g);
 * (K values; feasible is g_i <= 0), and its table is the library's: n_tab = W + K + 1 words per step,
 *   [ the user's row (W >= 0 words) | lambda_0 .. lambda_{K-1} | mu ],
 * n_tab <= ISLS_USER_MAX_TAB.  Where W > 0 both functions take `const P *row` (the W words) behind `par`, as a table cost's stage
 * does.  Every entry point that serves the cost (line search, expansion, value, sampling, isls_mpc_step_*) takes that table in
 * ztab / ztab_sb / nvia = n_tab as it takes any table, and costs a step with the augmented Lagrangian in the PHR form:
 *   c = stage ;  per i, h = lambda_i + mu g_i :  h > 0: c += lambda_i g_i + mu / 2 g_i^2 ;  else: c -= lambda_i^2 / (2 mu) (0 at mu = 0)
 * -- exactly `stage` at lambda = 0, mu = 0.  ISLS_ERR_UNSUPPORTED: n_con < 0, or n_con > 0 with n_tab < n_con + 1. */
int isls_user_cost_create_con(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t n_con, int32_t *id);
/* Constraints of the cost (0: a cost without), or ISLS_ERR_ARG for an id nobody registered. */
int isls_user_cost_n_con(int32_t id);
/* A 2-D field with derivatives for `stage` and `constraint`: a signed-distance map, a terrain height map, a risk map -- data of
 * 10^4 .. 10^6 words, shared by the batch and indexed by the state, which neither the parameters nor a table row can hold.  A
 * cost registered with n_field = C >= 1 channels of nx x ny samples may call, in both functions,
 *   isls::field(c, px, py)        c: a plain int channel (clamped to [0, C)); px, py: each an S or a plain number; the result an S
 * Sample [c, i, j] sits at (origin[0] + i spacing[0], origin[1] + j spacing[1]).  The interpolant is the tensor-product cubic
 * convolution with Keys' kernel at a = -1/2 (Catmull-Rom; csrc/user_field.hpp has the weights): C1, exact on the samples and on
 * polynomials up to degree 2 in each variable, first and second derivatives exact for every type of the contract.  Outside the
 * grid the field continues as a constant: the position is clamped per axis, and where the clamp acts the derivative along that
 * axis is zero.  The other arguments are those of isls_user_cost_create_con (n_tab = n_con = 0: neither).  A source that calls
 * isls::field in a cost registered WITHOUT a field does not compile (isls::field exists only in the programs of a field cost),
 * and the log ends with a sentence that says so.  The samples are never differentiated.
 * ISLS_ERR_UNSUPPORTED: n_field outside [1, ISLS_USER_MAX_FIELD], nx < 4, ny < 4, n_field * nx * ny > ISLS_USER_MAX_FIELD_WORDS.
 * Needs no GPU; the field's values come with isls_user_cost_set_field.  Unlike the other creates' ids, the id owns device memory. */
int isls_user_cost_create_field(const char *source, int32_t n, int32_t m, int32_t n_par, int32_t n_tab, int32_t n_con,
                                int32_t n_field, int32_t nx, int32_t ny, int32_t *id);
/* The values of the field: `values` [n_field, nx, ny] of dtype_of_values (ISLS_DTYPE_*) on the current device.  The library keeps
 * an fp64 and an fp32 copy in two buffers the registration owns on that device (allocated by the first call there; the copy of
 * the other precision is made by one small conversion kernel), and every later call overwrites them in place on `stream` -- no
 * compile, and no module's descriptor changes while origin and spacing stay what they were.  The first call on a device, and
 * one with another origin or spacing, also write the descriptor of every module of the cost loaded there, after what runs on
 * `stream` has ended (not inside a stream capture); modules loaded later get it as they load.
 * ISLS_ERR_ARG: an id nobody registered, a cost without a field, values / origin / spacing NULL, a spacing <= 0 or not finite.
 * ISLS_ERR_LAUNCH, before anything is enqueued: a first call on the device or a new grid while `stream` is capturing.
 * A NaN position gives NaN (value and derivatives; it reads cell 0, so no index leaves the buffers): under ISLS_RO_NAN_TO_1E5 a
 * diverged candidate of the line search is costed as one, as with any other stage.
 * Every launch that costs a step with a field cost (line search, expansion, value, multiplier update, sampling, isls_mpc_step_*,
 * isls_user_cost_grad_*) returns ISLS_ERR_ARG, before anything is launched, on a device where the field was never set. */
int isls_user_cost_set_field(int32_t id, const void *values, int32_t dtype_of_values, const double origin[2], const double spacing[2],
                             void *stream);
/* C, nx, ny of the cost's field (0, 0, 0: a cost without one); ISLS_ERR_ARG for an id nobody registered. */
int isls_user_cost_field_dims(int32_t id, int32_t *n_field, int32_t *nx, int32_t *ny);
/* The sample buffer of `dtype` on the current device (*ptr = NULL: not set there): it never moves once allocated.  ISLS_ERR_ARG:
 * no such id, a cost without a field. */
int isls_user_cost_field_ptr(int32_t id, int32_t dtype, void **ptr);
/* Lifetime: the two sample buffers (12 bytes per sample and device, about 200 MB at the limit) live until this call or the end of
 * the process -- the registry of user costs has no destroy.  isls_user_cost_release_field frees them on every device (it waits for
 * what still reads them); the registration, its programs and its loaded modules stay, the field is set nowhere afterwards (a
 * launch: ISLS_ERR_ARG), and the next isls_user_cost_set_field allocates again.  ISLS_ERR_ARG: no such id, a cost without a field. */
int isls_user_cost_release_field(int32_t id);
/* The multiplier and penalty update of such a cost along a trajectory, one launch for the batch (one wavefront per trajectory).
 * Per trajectory b with active[b] != 0 (NULL: all), with g = constraint(xhat_t, uhat_t) and the mu the table came with:
 *   g_out[b, t, i] = g_i (g_out nullable) ;  v_t = max_i max(0, g_i), +inf where a g_i is NaN ;  viol[b] = max_t v_t ;
 *   update != 0:  lambda_i <- max(0, lambda_i + mu g_i) (a NaN g_i leaves its lambda_i), and then, where
 *                 viol[b] > eta * viol_prev[b]:  mu <- min(phi mu, mu_max) in every row ;
 *   viol_prev[b] <- viol[b].
 * update == 0 leaves the table as it is.  tab is [B, N, n_tab] with tab_sb = N * n_tab (the multipliers belong to a trajectory);
 * cost_par [n_par] (cost_par_sb = 0) or [B, n_par].  ISLS_ERR_ARG: a cost without constraints, NULL arrays, another tab_sb,
 * update with phi < 1, mu_max < 0 or eta < 0. */
typedef struct isls_constraint_update_args {
    int32_t B, N, n, m;
    int32_t cost_model;      /* the cost's id */
    int32_t update;
    const void *cost_par;
    int64_t cost_par_sb;
    void *tab;
    int64_t tab_sb;
    const void *xhat, *uhat; /* [B,N,n], [B,N,m] */
    void *viol, *viol_prev;  /* [B] */
    void *g_out;             /* [B,N,n_con], nullable */
    double eta, phi, mu_max;
    const int32_t *active;   /* [B], nullable */
} isls_constraint_update_args;
int isls_user_constraint_update_f64(const isls_constraint_update_args *a, void *stream);
int isls_user_constraint_update_f32(const isls_constraint_update_args *a, void *stream);
/* The compile log of the cost's programs (as isls_user_model_log). */
int64_t isls_user_cost_log(int32_t id, char *buf, int64_t len);
/* The gfx950 code object of the cost with `model` (a built-in model of the cost's (n, m), a user model of them, or -1: the
 * expansion and the value only) for dtype, as isls_user_model_code.  Compiles the (cost, model, dtype) program if need be. */
int isls_user_cost_code(int32_t id, int32_t model, int32_t dtype, void *buf, int64_t *len);
/* Compiles the (cost, model, dtype) program if need be and loads its module onto the current device (once; outside any stream
 * capture).  A launch with a pair that has not been loaded compiles and loads it then, and fails inside a stream capture. */
int isls_user_cost_load(int32_t id, int32_t model, int32_t dtype);
/* cost[r] = sum_t stage(x[r,t], u[r,t], par, t, N): x [R,N,n], u [R,N,m], par [n_par] (par_sb = 0) or [R,n_par] -> cost [R]. */
int isls_user_cost_value_f64(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *x, const void *u,
                             void *cost, void *stream);
int isls_user_cost_value_f32(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *x, const void *u,
                             void *cost, void *stream);
/* The same for a cost with a table: tab [N,n_tab] (tab_sb = 0) or [R,N,n_tab] (tab_sb = N * n_tab); ISLS_ERR_ARG for tab == NULL
 * or another tab_sb, before any launch.  (isls_user_cost_value_* on a cost with a table: ISLS_ERR_ARG.) */
int isls_user_cost_value_tab_f64(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *tab, int64_t tab_sb,
                                 const void *x, const void *u, void *cost, void *stream);
int isls_user_cost_value_tab_f32(int32_t id, int32_t R, int32_t N, const void *par, int64_t par_sb, const void *tab, int64_t tab_sb,
                                 const void *x, const void *u, void *cost, void *stream);
/* The expansion of a user cost about the nominal, in the layouts and with the `active` semantics of isls_expand_quadratic_*:
 *   c0x, c0u = gradient ; Cxx = H_xx + 2 Qr ; Cuu = H_uu + 2 Rr ; Cux [B,N,m,n] = H_ux ; cost[b] (nullable) = the nominal's cost.
 * Cxx, Cuu, Cux nullable (skipped).  a->cost_model is the cost's id; Qtab, ztab, seq, u_std, q_nonzero are ignored. */
int isls_user_cost_expand_f64(const isls_expand_args *a, void *Cux, void *stream);
int isls_user_cost_expand_f32(const isls_expand_args *a, void *Cux, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Gradients of the nominal's cost by an adjoint sweep.  J = sum_{t=0}^{N-1} c_t(x_t, u_t) with x_0 given and x_{t+1} =
 * f(x_t, u_t, row_t) for t <= N-2 (u_{N-1} is costed and steps nothing, as in the line search).  With A_t, B_t of isls_linearize_*
 * and c0x, c0u of an expansion about the same nominal (no ADMM weights: Qr, Rr are not part of J), the TOTAL derivative of J at
 * fixed controls is
 *   lam_{N-1} = c0x_{N-1} ;   lam_t = c0x_t + A_t' lam_{t+1}   (t = N-2 .. 0)
 *   gu_t = c0u_t + B_t' lam_{t+1}   (t <= N-2) ;   gu_{N-1} = c0u_{N-1} ;   gx0 = lam_0
 * (each product summed from zero in index order, then added to the cost term).  A, Bm: views with any batch and time stride (a
 * batch stride of 0: one pair for the batch); c0x [B,N,n], c0u [B,N,m] dense; lam [B,N,n], gu [B,N,m], gx0 [B,n] (nullable).  A
 * trajectory with active[b] == 0 is left untouched in all three.  Served for every fast pair and for the generic pairs (n <= 16,
 * m <= 8); ISLS_ERR_UNSUPPORTED beyond, ISLS_ERR_ARG for a NULL array or a negative stride.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_adjoint_args {
    int32_t B, N, n, m;
    isls_view A, Bm;
    const void *c0x, *c0u;
    void *lam, *gu;
    void *gx0;                      /* nullable */
    const int32_t *active;          /* [B], nullable */
} isls_adjoint_args;
int isls_adjoint_sweep_f64(const isls_adjoint_args *a, void *stream);
int isls_adjoint_sweep_f32(const isls_adjoint_args *a, void *stream);

/* The directions of J that the sweep does not reach: the parameters and the per-step tables of a user model and a user cost.
 * They come from a program of their own per source and dtype, built on first request (isls_user_*_grad_build; needs no GPU): it
 * instantiates the source with S = P = a forward-mode dual number -- x, u constants, one word of [par | row] seeded -- so a source
 * must keep to the S contract of csrc/user_model_ad.hpp in what it does with `par` and `row` as well (no cast of them to an
 * integer, no plain-number temporaries of them).  A source that does not keeps working everywhere else: only this build fails,
 * ISLS_ERR_COMPILE, with the compiler's messages and that sentence in the source's log.  No other program of the source changes.
 *   model:  g_par[b,p] = sum_{t <= N-2} lam_{t+1}' df/dpar_p (x_t, u_t, row_t) ;  g_tab[b,t,w] = lam_{t+1}' df/drow_w  (row N-1: 0)
 *   cost:   g_par[b,p] = sum_t dc_t/dpar_p ;                                      g_tab[b,t,w] = dc_t/drow_w
 * One wavefront per (trajectory, direction); its lanes stride over the steps and the sum over t is a wave reduction in a fixed
 * order (no atomics: two launches give the same bits).  par / par_sb: the model's block [par | rows] as in isls_linearize_args
 * (its table is read from there), or the cost's parameters; tab / tab_sb: the cost's table as in isls_expand_args.ztab (unused
 * for a model).  A cost with constraints is differentiated in its PHR-augmented form at the multipliers in the table; only the
 * user's W words of a row are directions (g_tab [B,N,W]), the multipliers and mu are constants.  g_par [B,n_par], g_tab
 * [B,N,W]: either may be NULL (not computed).  Per-trajectory outputs also where par / tab are shared: the caller sums.
 * lam: the costate [B,N,n] of isls_adjoint_sweep_* (model only).  active as above. */
typedef struct isls_user_grad_args {
    int32_t B, N, n, m;
    int32_t id;                     /* the model's or the cost's id */
    int32_t _pad;
    const void *par; int64_t par_sb;
    const void *tab; int64_t tab_sb;
    const void *xhat, *uhat;        /* [B,N,n], [B,N,m] */
    const void *lam;
    void *g_par, *g_tab;
    const int32_t *active;
} isls_user_grad_args;
int isls_user_model_grad_build(int32_t id, int32_t dtype);
int isls_user_cost_grad_build(int32_t id, int32_t dtype);
int isls_user_model_grad_f64(const isls_user_grad_args *a, void *stream);
int isls_user_model_grad_f32(const isls_user_grad_args *a, void *stream);
int isls_user_cost_grad_f64(const isls_user_grad_args *a, void *stream);
int isls_user_cost_grad_f32(const isls_user_grad_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Monte-Carlo validation of a batch of controllers: M closed loops of each of P problems through its forward model and its own
 * controller, from random (or given) initial states and under random (or given) process noise, in one launch
 * (get_trajectory_sls, isls/isls_base.py:28-42 and isls/sls_base.py:91-105; get_trajectory_dp / _batch, isls/sls_base.py:61-89):
 *   dx_j = x_j - xhat_j ;  K_form 0:  u_i = (K_i dx_i + k_i) + uhat_i                         K [P,N,m,n],     k [P,N,m]
 *                          K_form 1:  u_i = ((K [dx_0 .. dx_i, 0 ..])_i + k_i) + uhat_i        K [P, N m, N n], k [P, N m]
 *   x_{i+1} = f(x_i, u_i) + w_i       (the control first, then the step, then the noise: the reference's order)
 * Every sum runs over j ascending from 0; entries of a dense K right of block i are never read.  xhat / uhat NULL: 0 (absolute
 * form).  A batch stride (`_sb`, in elements) of 0 shares the operand over the problems: K_sb == k_sb == 0 is one controller for
 * all of them.  model / model_par / par_sb as in isls_dense_loop_args / isls_rollout_args (built-in ids, user-model ids); the
 * families of csrc/families.def run at their own dimensions, ISLS_MODEL_LTI (par = [A(n*n), B(n*m)]) at any n <= 16, m <= 8.
 * Initial states: x0s [P,M,n] (explicit), or x0 [P,n] (stride x0_sb) with x0_std [n] (nullable: no spread):
 *   x0 = mean + x0_std o z.  Noise: none, w [P,M,N,n] (explicit; w_{N-1} is read and unused), or noise_std [n] with `seed`:
 *   w_i = noise_std o z.  The normals z are Philox4x32-10 / Box-Muller draws that depend on (seed, problem0 + problem,
 *   sample0 + sample, step, coordinate) only -- not on the launch shape or on how a caller cuts P or M into chunks: the layout is
 *   part of this ABI, written out in csrc/philox.hpp.  The normals are fp64; the _f32 entry point rounds std * z and
 *   mean + std * z once.  32-bit uniforms cut the tails at about 6.8 sigma.
 * Bounds (views [.,.,m] / [.,.,n]; each nullable: that side is free; sb / st = 0 shares them over problems / steps) and the
 * statistics, each nullable:
 *   viol_u int32 [P,N,m], viol_x int32 [P,N,n]: samples with u_i[c] < u_lo or > u_hi (x likewise) at that step and coordinate;
 *   viol_any int32 [P]: samples with any violation anywhere (of the bounds given);
 *   u_min, u_max [P,N,m], x_min, x_max [P,N,n]: extrema over the samples.
 *   They are ACCUMULATED (integer atomic adds, atomic min / max: order-independent, the same bits whatever the launch shape):
 *   THE CALLER ZEROES THE COUNTS and sets the minima to +inf, the maxima to -inf before the first launch; chunks over M add up.
 * Trajectories, each nullable (all NULL: statistics only): x_log [P,M,N,n], u_log [P,M,N,m], w_out [P,M,N,n] (the noise used;
 * written only when there is noise), x0_out [P,M,n].
 * work: caller-owned scratch of isls_mc_work_elems(...) elements (0 for K_form 0), opaque; work_elems its size.
 * ISLS_ERR_ARG before any launch: a NULL model_par / K / k, both or neither of x0s and x0 (or x0s with x0_std), w together with
 * noise_std, P < 0, M < 0, N < 1, n outside [1,16], m outside [1,8], K_form not 0 / 1, a negative stride, K_form 1 with work
 * NULL or work_elems too small.  ISLS_ERR_UNSUPPORTED: a model without a kernel at (n, m).
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_mc_loop_args {
    int32_t P, M, N, n, m;
    int32_t model;
    int32_t K_form;
    int32_t _pad;
    const void *model_par;
    int64_t par_sb;
    const void *K, *k;
    int64_t K_sb, k_sb;
    const void *xhat, *uhat;        /* [.,N,n], [.,N,m] nullable */
    int64_t xhat_sb, uhat_sb;
    const void *x0s;                /* [P,M,n], or NULL with: */
    const void *x0;                 /* [.,n] mean */
    int64_t x0_sb;
    const void *x0_std;             /* [n] nullable */
    const void *w;                  /* [P,M,N,n] nullable */
    const void *noise_std;          /* [n] nullable */
    uint64_t seed;
    int32_t problem0, sample0;      /* counter offsets of this launch's first problem / sample (a caller's chunks) */
    isls_view u_lo, u_hi;           /* [.,.,m] */
    isls_view x_lo, x_hi;           /* [.,.,n] */
    int32_t *viol_u, *viol_x, *viol_any;
    void *u_min, *u_max, *x_min, *x_max;
    void *x_log, *u_log, *w_out, *x0_out;
    void *work;
    int64_t work_elems;
} isls_mc_loop_args;

/* elements of the scratch buffer of isls_mc_closed_loop_* (0 for K_form 0 and for invalid dimensions) */
int64_t isls_mc_work_elems(int32_t P, int32_t M, int32_t N, int32_t n, int32_t m, int32_t K_form);

int isls_mc_closed_loop_f64(const isls_mc_loop_args *a, void *stream);
int isls_mc_closed_loop_f32(const isls_mc_loop_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One control step of a receding-horizon (model-predictive) loop for a batch of B plans, in one launch and in place: the first
 * control of every plan goes through the plant, the plan moves up by one step with its last row held, and it is rolled out again
 * from the measured state.  It restates, on the device, what a host loop does with the nominal_values setter
 * (isls/isls_base.py:80-85: the shifted plan becomes the nominal) around a closed-loop step in the reference's order
 * (isls/isls_base.py:59-75: the control first, then the step, then the noise), as isls_mc_closed_loop_* does.  Per trajectory b:
 *   1. x_m = xhat[b,0] ;  u_a = min(max(uhat[b,0], u_lo), u_hi) ;  x+ = f(x_m, u_a; plant_par_b) + w_b
 *      w_b: none, w [B,n] (explicit), or noise_std o z with the normals z of csrc/philox.hpp at (seed, problem0 + b, sample 0,
 *      step, coordinate) -- the draws of isls_mc_closed_loop_* at the same counters; the _f32 entry rounds std * z once.
 *   2. for a in xhat, uhat, K, zx, zu:  a~[t] = a[t+1] (t < N-1), a~[N-1] = a[N-1];  the table likewise, its last row tab_next
 *      where that is given.  A shared table (tab_sb == 0) is moved once per launch, not once per trajectory.
 *   3. x_0 = x+ ;  t = 0 .. N-1:  u_t = (K~_t (x_t - x~_t)) + u~_t  (K NULL: u_t = u~_t) ;  t < N-1:  x_{t+1} = f(x_t, u_t; model_par_b)
 *      Every sum runs over j ascending from 0, every multiply-add of it is one fused operation.
 *   4. xhat <- x, uhat <- u, K <- K~, zx <- zx~, zu <- zu~, the table, and the outputs x_meas_out = x_m, u_out = u_a, x_next_out = x+.
 *   N == 1: nothing moves (row 0 is the held row): x_0 = x+, u_0 = (K_0 (x+ - xhat_0)) + uhat_0.
 * All pointers are device pointers; `_sb` are batch strides in elements, 0 = shared.  model / model_par / par_sb as in
 * isls_mc_loop_args (the solver's model: the families of csrc/families.def at their own dimensions, ISLS_MODEL_LTI at any
 * n <= 16, m <= 8, user-model ids); plant_par / plant_sb: the same model with the plant's parameters (NULL: model_par).
 * In/out: xhat [B,N,n], uhat [B,N,m]; K [B,N,m,n] (nullable: open-loop re-roll); zx [B,N,n], zu [B,N,m] (each nullable: not
 * moved); tab [N,W] (tab_sb = 0) or [B,N,W] (tab_sb = N W), nullable, with tab_next [W] / [B,W] (tab_next_sb = 0 / W; nullable:
 * the last row is held).  u_lo, u_hi [m] (each nullable: that side is free) clip the APPLIED control only.
 * Outputs, each nullable: x_meas_out [B,n], u_out [B,m], x_next_out [B,n], each with a batch stride of its own (a caller points
 * them at column s of its [B,T,.] logs).  Nothing else is written.
 * ISLS_ERR_ARG before any launch: a NULL xhat / uhat / model_par, B < 0, N < 1, n outside [1,16], m outside [1,8], a negative
 * stride, tab with W outside [1,16], w together with noise_std.  ISLS_ERR_UNSUPPORTED: a model without a kernel at (n, m).
 * B == 0: ISLS_OK, nothing is launched.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_mpc_step_args {
    int32_t B, N, n, m;
    int32_t model;
    int32_t W;                      /* words per row of the table */
    const void *model_par;
    int64_t par_sb;
    const void *plant_par;          /* nullable: model_par */
    int64_t plant_sb;
    void *xhat, *uhat;              /* [B,N,n], [B,N,m] */
    void *K;                        /* [B,N,m,n] nullable */
    void *zx, *zu;                  /* [B,N,n], [B,N,m] nullable */
    void *tab;                      /* [.,N,W] nullable */
    int64_t tab_sb;
    const void *tab_next;           /* [.,W] nullable */
    int64_t tab_next_sb;
    const void *u_lo, *u_hi;        /* [m] nullable */
    const void *w;                  /* [B,n] nullable */
    const void *noise_std;          /* [n] nullable */
    uint64_t seed;
    int32_t problem0, step;         /* counter offset of this launch's first trajectory; the control step */
    void *x_meas_out, *u_out, *x_next_out;
    int64_t x_meas_sb, u_out_sb, x_next_sb;
} isls_mpc_step_args;

int isls_mpc_step_f64(const isls_mpc_step_args *a, void *stream);
int isls_mpc_step_f32(const isls_mpc_step_args *a, void *stream);

/* ---------------------------------------------------------------------------------------------
 * One sampling round about the nominal of a batch of B problems (a warm start of the MPPI kind: model-predictive path integral
 * control), in two launches and in place.  The reference has no counterpart: its solvers refine the nominal they are handed
 * (isls/isls.py:336-374) and end in the nearest local minimum.  Per problem b, with S samples:
 *   1. eps[0,t,:] = 0 ;  s >= 1:  eps[s,t,:] = sigma_b o z,  z the normals of csrc/philox.hpp at (seed, problem0 + b, sample s,
 *      step t, coordinate) -- the draws of isls_mc_closed_loop_* at the same counters; the _f32 entry rounds sigma * z once.
 *   2. u[s,t] = min(max(uhat[b,t] + eps[s,t], u_lo), u_hi) ;  e[s,t] = u[s,t] - uhat[b,t] ;  x[s,0] = xhat[b,0],
 *      x[s,t+1] = f(x[s,t], u[s,t]; model_par_b)  (open loop).
 *   3. costs[b,s] = the cost of (x[s], u[s]) as isls_rollout_ls_* counts it for cost_model, by the same code: the via-point cost
 *      sum_t (x_t-z_t)'Q_t(x_t-z_t) + u_std |u_t|^2, ISLS_COST_PHUBER (ISLS_MODEL_TASSA), or a user cost's sum of `stage` with its
 *      table row; u_{N-1} is costed, no ADMM terms.  A NaN is written as +inf.  There is no q_nonzero hint here: the via-point
 *      term is evaluated at every step, so a state that has overflowed to +-inf gives 0 * inf = NaN (hence +inf) also where
 *      Q_t == 0, a step the line search's hint would skip.
 *   4. Smin = min_s costs[b,s], smin its FIRST index ;  w_s = exp(-(costs[b,s] - Smin) / (temperature max(Smin, tiny))) / sum of
 *      the same (tiny: the smallest normal number of the precision) ;  u_new[t] = uhat[b,t] + sum_s w_s e[s,t] ;  ess = 1 / sum w_s^2.
 *   5. x_new = the rollout of u_new, c_new its cost.  c_new < Smin: (xhat, uhat)[b] <- (x_new, u_new), cost_after = c_new,
 *      took_best = 0.  Otherwise (also c_new NaN): (xhat, uhat)[b] <- (x[smin], u[smin]), cost_after = Smin, took_best = 1.
 *      So cost_after <= cost_before = costs[b,0], the cost of the nominal controls rolled out from xhat[b,0].
 *   xhat[b,0] is never written.  costs[b,0] not finite: the problem is left as it is, cost_before = cost_after = costs[b,0],
 *   cost_best = Smin, ess = 0, took_best = 0 (the caller decides; iSLS.sample_nominal raises).
 * Minimum, arg-min and every sum over the samples are taken in a fixed order: the results are bitwise repeatable and do not depend
 * on B or on the other problems of the launch.  The draws are never stored: step 4 generates them again.  problem_ids [B] gives
 * every problem the counter of its own draws (a subset of a larger batch repeats that batch's numbers); phase splits the call
 * into its two launches (1: steps 1-3, 2: steps 4-5 on the costs as they stand) for tools that time them apart.
 * All pointers are device pointers; `_sb` are batch strides in elements, 0 = shared.  model / model_par / model_par_sb, cost_model /
 * cost_par / cost_par_sb, Qtab / ztab / seq / u_std / nvia as in isls_rollout_args (a user cost's table in ztab / ztab_sb / nvia).
 * The families of csrc/families.def, user models and user costs; fast (n, m) pairs only.
 * In/out: xhat [B,N,n], uhat [B,N,m].  sigma [m] (sigma_sb = 0) or [B,m] (sigma_sb = m), >= 0.  u_lo, u_hi [m], each nullable (that
 * side is free).  active [B] nullable: a problem with active[b] == 0 is skipped, nothing of it is read or written.
 * Workspace and output: costs [B,S] (caller allocated).  Statistics, each nullable, element b at b * stat_sb (a caller points them
 * at column r of its [B, rounds] logs): cost_before, cost_after, cost_best (= Smin), ess; took_best (int32).
 * ISLS_ERR_ARG before any launch: a NULL xhat / uhat / model_par / sigma / costs, B < 0, N < 1, S < 1, n < 1, m < 1, a negative
 * stride, phase outside [0,2], temperature not a positive finite number, a via-point cost without its tables, a user cost without cost_par or with
 * table fields that do not fit its registration.  ISLS_ERR_UNSUPPORTED: (n, m) without the row-per-lane kernels, a model without
 * a family at (n, m), ISLS_COST_PHUBER with another model than ISLS_MODEL_TASSA, N m words (plus a dense LTI model's) beyond the
 * 48 KB of LDS the update keeps u_new in, B ceil(S / 64) >= 2^31.  B == 0: ISLS_OK, nothing is launched.
 * ------------------------------------------------------------------------------------------- */
typedef struct isls_sample_args {
    int32_t B, N, n, m, S;
    int32_t model;
    int32_t cost_model;
    int32_t nvia;
    const void *model_par;
    int64_t model_par_sb;
    const void *cost_par;
    int64_t cost_par_sb;
    void *xhat, *uhat;              /* [B,N,n], [B,N,m] */
    const void *Qtab;               /* [.,nvia,n,n] */
    int64_t Qtab_sb;
    const void *ztab;               /* [.,nvia,n]; a user cost's table [.,N,W] */
    int64_t ztab_sb;
    const int32_t *seq;             /* [N] */
    double u_std;
    const void *sigma;              /* [.,m] */
    int64_t sigma_sb;
    const void *u_lo, *u_hi;        /* [m] nullable */
    double temperature;
    uint64_t seed;
    int32_t problem0;               /* counter offset of this launch's first problem */
    int32_t phase;                  /* 0: both launches; 1: the costs only; 2: the update only, on costs [B,S] as they stand */
    const int32_t *problem_ids;     /* [B] nullable: the problem counter of each problem's draws (else problem0 + b) */
    const int32_t *active;          /* [B] nullable */
    void *costs;                    /* [B,S] */
    void *cost_before, *cost_after, *cost_best, *ess;
    int32_t *took_best;
    int64_t stat_sb;
} isls_sample_args;

int isls_sample_nominal_f64(const isls_sample_args *a, void *stream);
int isls_sample_nominal_f32(const isls_sample_args *a, void *stream);

/* The same round in CLOSED LOOP about feedback gains (iLQG-guided / tube MPPI): noise injected at step t is corrected at the steps
 * behind it, so the samples stay near the nominal, where the model and the gains are valid.  K [.,N,m,n] are the gains G_t = K[b,t]
 * (K_sb = 0: shared by the batch; N m n: per problem); the anchors xa = xhat[b], ua = uhat[b] are the nominal as it stands when the
 * launch begins.  `a` is read as by isls_sample_nominal_* (phase, active, problem_ids and the statistics mean the same) and the
 * draws come from the same counters: a closed-loop and an open-loop round with one seed see the same noise.  Per problem b:
 *   1. eps[s,t,:] as above (sample 0: zero).
 *   2. x[s,0] = xa_0 ;  u[s,t] = min(max((ua_t + G_t (x[s,t] - xa_t)) + eps[s,t], u_lo), u_hi) ;  x[s,t+1] = f(x[s,t], u[s,t]).
 *      The feedback product is summed over the state index ascending and added to ua_t first; the drawn noise is then added with
 *      a sum that is never contracted.
 *   3. costs[b,s] as above, by the same code; a NaN is written as +inf.
 *   4. Smin, smin, w_s, ess as above (the same fixed order) ;  d_t = sum_s w_s eps[s,t] -- the DRAWN noise, not the realised clipped
 *      deviation: that depends on the sample's state and could not be generated again without its rollout, the draw can.
 *   5. The candidate is the closed-loop rollout of v_t = ua_t + d_t from xa_0: u_new_t = min(max(v_t + G_t (x_new_t - xa_t), u_lo),
 *      u_hi), c_new its cost.  c_new < Smin: (xhat, uhat)[b] <- (x_new, u_new), cost_after = c_new, took_best = 0.  Otherwise (also
 *      c_new NaN): sample smin is rolled out again in closed loop from its regenerated draws, (xhat, uhat)[b] <- (x[smin], u[smin]),
 *      cost_after = Smin, took_best = 1.  What is stored are the realised states and the realised, clipped controls: the new nominal
 *      is dynamically consistent and inside the clip.  cost_before = costs[b,0]: the cost of the nominal itself where it is
 *      consistent and inside the clip (sample 0 then never leaves it).
 *   xhat[b,0] is never written; a costs[b,0] that is not finite leaves the problem as it is, with the statistics as above.
 * The update keeps the new states and controls in LDS until the choice is made (the anchors are needed until then).
 * ISLS_ERR_ARG before any launch: a NULL K, a negative K_sb, and everything isls_sample_nominal_* refuses.  ISLS_ERR_UNSUPPORTED: as
 * above, the LDS limit being N (n + m) words (plus a dense LTI model's) within the same 48 KB. */
int isls_sample_nominal_fb_f64(const isls_sample_args *a, const void *K, int64_t K_sb, void *stream);
int isls_sample_nominal_fb_f32(const isls_sample_args *a, const void *K, int64_t K_sb, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Closed-loop covariance of a batch of stage-local controllers: the analytic counterpart of isls_mc_closed_loop_*.  The
 * reference has no covariance code (it samples, or constrains phi_u S0 phi_u' in its SLS form); this is the first and second
 * moment of the LINEARISED closed loop x_{t+1} = f(x_t, u_t) + w_t, u_t = uhat_t + k_t + K_t (x_t - xhat_t) about a nominal
 * that is dynamically consistent (xhat_{t+1} = f(xhat_t, uhat_t)), with x_0 ~ (xhat_0 + dx0, S0) and w_t ~ (0, W_t):
 *   Sig_0 = (S0 + S0')/2 ;  d_0 = dx0 ;  for t = 0 .. N-1, with Phi_t = A_t + B_t K_t:
 *     xbar_t = xhat_t + d_t ;  ubar_t = uhat_t + (k_t + K_t d_t) ;  Su_t = sym(K_t Sig_t K_t')
 *     d_{t+1} = Phi_t d_t + B_t k_t ;  Sig_{t+1} = sym(Phi_t Sig_t Phi_t' + W_t) ,  sym(S) = (S + S')/2 entry by entry
 *   (W_t is added BEHIND step t, the convention of isls_mc_closed_loop_*; W_{N-1} acts on nothing).  Every covariance written is
 *   exactly symmetric and x_var / u_var are the diagonals of x_cov / u_cov bit for bit.  Every multiply-add is one fused
 *   operation and every sum runs over its inner index ascending (csrc/covariance.hip writes the order out).
 * Inputs.  A [.,.,n,n], Bm [.,.,n,m]: views (sb = st = 0: a shared LTI pair).  K [.,N,m,n] (K_sb = 0: one controller for all);
 * k [.,N,m] nullable (0);  xhat [.,N,n], uhat [.,N,m] nullable (0);  dx0 [.,n] nullable (0);  S0 [.,n,n];  W [.,.,n,n] view,
 * nullable (no noise; sb = 0 / st = 0 shares it over problems / steps).  `_sb` are batch strides in elements, 0 = shared.
 * Bounds u_lo, u_hi [.,.,m], x_lo, x_hi [.,.,n]: views as in isls_mc_loop_args, each nullable (that side is free).
 * Outputs, each nullable: x_mean [P,N,n], u_mean [P,N,m], x_var [P,N,n], u_var [P,N,m], x_cov [P,N,n,n], u_cov [P,N,m,m] and
 *   p_x [P,N,n], p_u [P,N,m]: the Gaussian probability of lying outside [lo, hi] at that step and coordinate,
 *   p = erfc((mu - lo) / (sigma sqrt 2))/2 + erfc((hi - mu) / (sigma sqrt 2))/2 (an absent or infinite side contributes 0);
 *   sigma == 0 exactly (a variance <= 0): p = 1 where mu < lo or mu > hi, else 0.
 * Problems with active[b] == 0 are skipped: nothing of theirs is written.
 * The (n, m) pairs of csrc/families.def only (isls_dims_supported), any other pair: ISLS_ERR_UNSUPPORTED.  ISLS_ERR_ARG: a NULL
 * A, Bm, K or S0, N < 1, P < 0, a negative stride.  P == 0: ISLS_OK, nothing is launched.  No scratch memory, no work buffer.
 * ------------------------------------------------------------------------------------------- */
#ifndef __HIPCC_RTC__   /* a host-side entry point: the device code compiled at run time (user models and costs) reads none of it */
typedef struct isls_cov_args {
    int32_t P, N, n, m;
    isls_view A, Bm;                /* [.,.,n,n], [.,.,n,m] */
    const void *K, *k;              /* [.,N,m,n], [.,N,m] (k nullable) */
    int64_t K_sb, k_sb;
    const void *xhat, *uhat;        /* [.,N,n], [.,N,m] nullable */
    int64_t xhat_sb, uhat_sb;
    const void *dx0;                /* [.,n] nullable: mean initial deviation x0 - xhat_0 */
    int64_t dx0_sb;
    const void *S0;                 /* [.,n,n] initial covariance */
    int64_t S0_sb;
    isls_view W;                    /* [.,.,n,n] nullable: process-noise covariance */
    isls_view u_lo, u_hi;           /* [.,.,m] */
    isls_view x_lo, x_hi;           /* [.,.,n] */
    const int32_t *active;          /* [P] nullable */
    void *x_mean, *u_mean, *x_var, *u_var, *x_cov, *u_cov, *p_u, *p_x;
} isls_cov_args;

int isls_cov_closed_loop_f64(const isls_cov_args *a, void *stream);
int isls_cov_closed_loop_f32(const isls_cov_args *a, void *stream);
#endif

int isls_version(void);
/* The gain memo of isls_ilqr_admm_outer_*.  Where a batch shares the inputs of the gain recursion (batch stride 0 on Cxx, Cuu,
 * Cux and on the parameter row of the structured ISLS_MODEL_DI form, sequential feed-forward passes), the driver keeps the one
 * table of records [K_t | fac_t] in device memory of the library's own, one entry per (device, stream, precision, n, m, N,
 * solve mode), together with a snapshot of every word the recursion read.  Each call compares the inputs with the snapshot on
 * the device, in stream order: equal bit patterns (and no NaN) -- the recursion is not run again, K and the first feed-forward
 * pass are produced from the kept table with the same arithmetic; anything else -- the recursion runs and the entry is
 * refreshed (never from a pass that met a pivot that is not positive).  Results are bit-identical either way; nothing is keyed
 * on addresses and there is no switch.  A capturing stream or a failed allocation: the call runs without the memo.
 * An empty batch (B = 0) launches nothing and touches no entry.
 * Limits.  An entry (the snapshot and N records: ~75 KB at n = 6, m = 3, N = 100 in double) belongs to a stream HANDLE and
 * lives until isls_gain_memo_clear: a program that keeps creating streams should call it when it destroys them (a recycled
 * handle that finds an old entry is harmless -- validity is by content).  One host thread drives a (stream, shape) pair at a
 * time, as for every stream-ordered call here: two threads enqueueing on the same stream and shape would share one `match`
 * word.  K is written with 16-byte stores (fp32: 8-byte), like the gain pass's own: K must be aligned accordingly.
 * isls_gain_memo_stats: device checks and matches so far, summed over the entries (synchronises: for tests and tools).
 * isls_gain_memo_clear: frees every entry after synchronising its device; no other thread may be inside
 * isls_ilqr_admm_outer_* meanwhile (a call in flight holds pointers into the entry). */
int isls_gain_memo_stats(int64_t *checks, int64_t *matches);
void isls_gain_memo_clear(void);
/* 1 when the kernels are instantiated for state dimension n and control dimension m (the pairs are compile-time template
 * arguments: csrc/isls_common.hpp ISLS_FOR_EACH_DIMS), else 0: every entry point returns ISLS_ERR_UNSUPPORTED for other pairs. */
int32_t isls_dims_supported(int32_t n, int32_t m);
/* 1 when (n, m) is served at all: every pair with n <= 16, m <= 8 (the reference takes any dimensions, isls/base.py:11-14).  Pairs
 * without an instantiation run the generic kernels (csrc/generic.hip: dimensions at run time, one trajectory per wavefront,
 * matrices in LDS; array form only -- no packed records, no time-parallel segments, dense LTI / double-integrator model,
 * via-point cost): isls_riccati_gain / isls_riccati_ff / isls_rollout_ls / isls_admm_update / isls_ilqr_admm_outer and the
 * streaming kernels work, the isls_columns_* entry points of isls_admm do not (ISLS_ERR_UNSUPPORTED). */
int32_t isls_dims_generic(int32_t n, int32_t m);
const char *isls_error_string(int code);
/* Per-kernel-family durations for bench.py: HIP events recorded on the launch stream around the launches that
 * isls_ilqr_admm_outer_* enqueues, kept in a CALLER-OWNED context (the library itself has no state): create one, put it
 * into isls_outer_args.timing, read it after the timed region, destroy it.  kind: 0 gain, 1 ff, 2 rollout, 3 admm,
 * 4 ff_prepare.  A context serves one host thread at a time. */
void *isls_timing_create(void);
void isls_timing_destroy(void *timing);
int isls_timing_reset(void *timing);                 /* start a new measurement window                          */
int isls_timing_pause(void *timing, int paused);     /* suspend / resume recording without resetting the window */
double isls_timing_read_ms(void *timing, int kind, int *count);   /* summed ms and launch count of one family; synchronises */

#ifdef __cplusplus
}
#endif
#endif /* ISLS_HIP_H */
