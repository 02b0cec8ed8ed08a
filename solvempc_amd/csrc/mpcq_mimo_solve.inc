// solvempc_amd/csrc/mpcq_mimo_solve.inc — the body of mimo_solve_kernel and mimo_solve_ref_kernel (mpcq_mimo.hip, which
// describes it), included into each: the kernel defines its argument `a` (MimoArgs), the template parameters NU, DK and
//   constexpr bool REF;  const double *ref;  long long ref_stride;
// REF: the step's reference is a horizon of N n_y values per QP (ref + b ref_stride) in place of a.yref.
    const int b = blockIdx.x;
    if (b >= a.batch) return;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    const int rg = t >> 3, cg = t & 7;
    const int N = a.N, nx = a.nx, ny = a.ny, n = N * NU, m = 2 * n;
    const MimoLayout L = MimoLayout::make(N, nx, NU, ny);
    const double *ops = a.ops + (size_t)b * a.ops_stride;
    const SolverSettings &st = a.st;
    // vector role: wave c = component, lane k = horizon block
    const int c = wv, k = lane;
    const bool valid = c < NU && k < N;
    const int e = valid ? k * NU + c : 0;  // natural index (masked when !valid)
    const int vi = c * 32 + (k & 31);      // component-major slot
    // ONE (n_u = 4, diagonal K0): the matrix rows are permuted so that wave c holds the rows of
    // component c, row group rg = 8 c + j register i = (block 4 j + i, component c): the GEMV output a
    // lane consumes is produced inside its own wave (a lane permute, no LDS round trip, no barrier),
    // and an iteration has one barrier (the rhs, double-buffered).  Otherwise row group rg holds the
    // natural rows 4 rg .. 4 rg + 3.
    constexpr bool ONE = NU == 4 && DK;
    // (r = rg laundered through an empty asm at the use: hoisted out of the solve loop, these
    // indices would hold registers the matrix needs)
    auto row_nat = [](int r, int i) { return ONE ? 16 * (r & 7) + 4 * i + (r >> 3) : 4 * r + i; };
    auto row_blk = [](int r, int i) { return ONE ? 4 * (r & 7) + i : (4 * r) / NU + i / NU; };
    auto row_cmp = [](int r, int i) { return ONE ? r >> 3 : i % NU; };
    auto rg_here = [&]() {
        int r = rg;
        if (ONE) asm volatile("" : "+v"(r));
        return r;
    };
    MPCQ_MSTAMP(0, __builtin_amdgcn_s_memtime());

    // GEMV inputs and the Gauss-Jordan row broadcast: natural order in 16-element segments padded to
    // 18 (kSegLd), so the 8 column groups' 16-B reads fall in distinct LDS banks; the GEMV output is
    // component-major (the vector role reads it lane-consecutively)
    __shared__ __attribute__((aligned(16))) double s_vec[2][kSegN];  // rhs (GEMV input; alternating in ONE)
    __shared__ __attribute__((aligned(16))) double s_nat[kSegN];   // warm start: x
    __shared__ __attribute__((aligned(16))) double s_out[kMimoN];  // GEMV output, component-major
    __shared__ __attribute__((aligned(16))) double s_row[2][2][kSegN];  // pivot rows k, k + 1 (alternating)
    __shared__ double s_D[kMimoN], s_E[kMimoN], s_K0[16], s_SW[32 * 16];  // D, E component-major
    __shared__ double s_xb[4][kMimoN];  // scan exchange buffers (rotated: a buffer is rewritten 4 barriers later)
    __shared__ double s_red[2][4][16];  // cross-wave reductions (alternating)
    // the checks' settings and the cost scaling, read from LDS where they are used: held in SGPRs
    // across the solve loop they spill into VGPR lanes that every iteration reloads
    // (read back through readfirstlane: the branches on them, some holding barriers, stay uniform)
    __shared__ double s_cfg[8];
    auto cfg = [&](int i) {
        const unsigned long long u = (unsigned long long)__double_as_longlong(s_cfg[i]);
        const unsigned lo = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)u);
        const unsigned hi = (unsigned)__builtin_amdgcn_readfirstlane((int)(unsigned)(u >> 32));
        return __longlong_as_double((long long)(((unsigned long long)hi << 32) | lo));
    };
    if constexpr (REF) {  // the front end's Fr ref term first, while nothing else is live: this QP's reference
                          // differences ref_i - ref_{i+1} (ref_N = 0), N n_y <= 384 doubles, staged in s_xb (idle until
                          // the first product), then this lane's sum parked in s_out (idle until the first GEMV).
                          // The plant's Frs (n n_y <= 1536 doubles) goes through LDS as well, one coalesced pass,
                          // not read from global a row per d where it is used (170.5 -> 169.1 ms per 262,144 plants)
        extern __shared__ double s_frs[];  // (dynamic: n n_y doubles, the launch sizes it)
        const double *rb = ref + (long long)b * ref_stride;
        double *dl = &s_xb[0][0];
        for (int i = t; i < N * ny; i += kMimoThreads) dl[i] = rb[i] - (i + ny < N * ny ? rb[i + ny] : 0.0);
        for (int i = t; i < n * ny; i += kMimoThreads) s_frs[i] = ops[L.Frs + i];
        __syncthreads();
        if (valid) {  // sum_d F[N-1-d] (ref_{k+d} - ref_{k+d+1}): ascending d, then ascending y
            double s2 = 0.0;
            for (int d = 0; d < N - k; d++) {
                const double *fd = s_frs + ((N - 1 - d) * NU + c) * ny, *dd = dl + (k + d) * ny;
#pragma unroll
                for (int i = 0; i < 12; i++)
                    if (i < ny) s2 = __builtin_fma(fd[i], dd[i], s2);
            }
            s_out[vi] = s2;
        }
        asm volatile("" ::: "memory");  // (the front end reloads it: no register held in between)
    }
    for (int i = t; i < kMimoN; i += kMimoThreads) {
        const int cc = i >> 5, kk = i & 31;
        const bool ok = cc < NU && kk < N;
        s_D[i] = ok ? ops[L.D + kk * NU + cc] : 1.0;
        s_E[i] = ok ? ops[L.E + kk * NU + cc] : 1.0;
    }
    for (int i = t; i < kSegN; i += kMimoThreads) s_vec[0][i] = s_vec[1][i] = s_nat[i] = 0.0;
    for (int i = t; i < 16; i += kMimoThreads) {
        const int r = i >> 2, cc = i & 3;
        s_K0[i] = (r < NU && cc < NU) ? ops[L.K0 + r * NU + cc] : 0.0;
    }
    for (int i = t; i < 32 * 16; i += kMimoThreads) {
        const int kk = i >> 4, ci = (i >> 2) & 3, cj = i & 3;
        s_SW[i] = (kk < N && ci < NU && cj < NU) ? ops[L.SW + (kk * NU + ci) * NU + cj] : 0.0;
    }

    const double c64 = ops[L.cs];
    if (t == 0) {
        s_cfg[0] = st.eps_abs; s_cfg[1] = st.eps_rel; s_cfg[2] = st.eps_prim_inf; s_cfg[3] = st.eps_dual_inf;
        s_cfg[4] = st.adaptive_rho_tolerance; s_cfg[5] = st.scaled_termination ? 1.0 : 0.0;
        s_cfg[6] = c64; s_cfg[7] = ops[L.cs + 1];
    }
    const double sigma = st.sigma, alpha = st.alpha, oma = 1.0 - st.alpha;
    const bool load = a.warm && !a.fresh;

    // this lane's element of the ADMM state (registers; the products exchange through s_xb)
    double vx = 0.0, vzt = 0.0, vzb = 0.0, vyt = 0.0, vyb = 0.0, vpx = 0.0, vqh = 0.0, vut = 0.0, vub = 0.0;
    double vrhs = 0.0, vdx = 0.0, vdpx = 0.0, vdyt = 0.0, vdyb = 0.0;
    const double vD = valid ? ops[L.D + e] : 1.0, vE = valid ? ops[L.E + e] : 1.0;
    // ---- the MPC front end: this lane's element of q and u, and the state
    int tchg = 0;
    {
        double q = 0.0, uth = 0.0, ubh = 0.0, x = 0.0, zt = 0.0, zb = 0.0, yt = 0.0, yb = 0.0;
        if (valid) {
            const double De = vD, Ee = vE;
            // setF (:372-375): q = Fx X + Fu U + Fr ref, ref = 1_N (x) yref (updateRef :378-380)
            double s0 = 0.0, s1 = 0.0, s2 = 0.0, kx = 0.0, k0u = 0.0;
            const double *fx = ops + L.Fx + (size_t)e * nx, *fr = ops + L.Frs + (size_t)e * ny;
            const double *Kc = ops + L.K + c * nx;
#pragma unroll
            for (int i = 0; i < 12; i++)
                if (i < nx) {
                    const double xv = a.X[(size_t)b * nx + i];
                    s0 = __builtin_fma(fx[i], xv, s0);
                    kx = __builtin_fma(Kc[i], xv, kx);
                }
            if constexpr (REF) {
                s2 = s_out[vi];  // (formed first thing, above)
            } else {
#pragma unroll
                for (int i = 0; i < 12; i++)
                    if (i < ny && a.yref) s2 = __builtin_fma(fr[i], a.yref[i], s2);
            }
#pragma unroll
            for (int i = 0; i < NU; i++) {
                const double uv = a.U[(size_t)b * NU + i];
                s1 = __builtin_fma(ops[L.Fu + (size_t)e * NU + i], uv, s1);
                k0u = __builtin_fma(ops[L.K0 + c * NU + i], uv, k0u);
            }
            q = s0 + s1 + s2;
            if (a.q_out) a.q_out[(size_t)b * n + e] = q;
            q = (q * De) * c64;
            // (:93-99): u = W0 + Sbar X + Ku U; Sbar block rows k < s_rows = [K; -K]; Ku = [-K0; K0]
            if (!(k < a.s_rows)) kx = 0.0;
            const double w0 = ops[L.w0 + c];
            const double utop = w0 + kx + -k0u, ubot = w0 + -kx + k0u;
            if (a.u_out) {
                a.u_out[(size_t)b * m + e] = utop;
                a.u_out[(size_t)b * m + n + e] = ubot;
            }
            uth = utop * Ee;
            ubh = ubot * Ee;
            // l = -DBL_MAX (:42): every row stays an inequality while u^ is finite
            if (!(uth < kInfty * kMinScaling) || !(ubh < kInfty * kMinScaling)) tchg = 1;
            if (load) {
                x = a.xs[(size_t)b * n + e];
                zt = a.zs[(size_t)b * m + e];
                zb = a.zs[(size_t)b * m + n + e];
                yt = a.ys[(size_t)b * m + e];
                yb = a.ys[(size_t)b * m + n + e];
            }
            s_nat[seg_of(e)] = x;
        }
        vqh = q; vut = uth; vub = ubh;
        vx = x; vzt = zt; vzb = zb; vyt = yt; vyb = yb;
    }
    int status = __syncthreads_or(tchg) ? kTypeChanged : kUnsolved;
    double rho = a.fresh ? fmin(fmax(st.rho, kRhoMin), kRhoMax) : a.rhos[b];
    MPCQ_MSTAMP(1, __builtin_amdgcn_s_memtime());

    // ---- vector products (every thread calls them: each holds one barrier)
    int xb = 0;
    auto scan_x = [&](double v, bool suffix) -> const double * {
        double *buf = s_xb[xb];
        xb = (xb + 1) & 3;
        const double p = suffix ? lane_ssum(v, lane) : lane_psum(v, lane);
        if (k < 32) buf[vi] = p;
        return buf;
    };
    auto mix_plain = [&](const double *buf) {  // sum_c' K0[c][c'] buf[c'][k]
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < NU; j++) acc = __builtin_fma(s_K0[(c & 3) * 4 + j], buf[j * 32 + (k & 31)], acc);
        return acc;
    };
    auto mix_trans = [&](const double *buf) {  // sum_r K0[r][c] buf[r][k]
        double acc = 0.0;
#pragma unroll
        for (int j = 0; j < NU; j++) acc = __builtin_fma(s_K0[j * 4 + (c & 3)], buf[j * 32 + (k & 31)], acc);
        return acc;
    };
    // (A^ x)_top = E (L (x) K0) D x (the bottom half is its negation); x = this lane's element.  With
    // every K0 diagonal (DK) the products are lane-local scans: no exchange, no barrier.
    const double k0cc = s_K0[(c & 3) * 5];
    auto A_of = [&](double xv) {
        if constexpr (DK) {
            const double p = lane_psum(valid ? vD * xv : 0.0, lane);
            return valid ? vE * (k0cc * p) : 0.0;
        } else {
            const double *bf = scan_x(valid ? vD * xv : 0.0, false);
            __syncthreads();
            return valid ? vE * mix_plain(bf) : 0.0;
        }
    };
    // A^' [w_top; w_bot] = D (L (x) K0)' E d, d = w_top - w_bot
    auto At_of = [&](double d) {
        if constexpr (DK) {
            const double p = lane_ssum(valid ? vE * d : 0.0, lane);
            return valid ? vD * (k0cc * p) : 0.0;
        } else {
            const double *bf = scan_x(valid ? vE * d : 0.0, true);
            __syncthreads();
            return valid ? vD * mix_trans(bf) : 0.0;
        }
    };
    auto At_of2 = [&](double d1, double d2, double &o1, double &o2) {
        const double E = valid ? vE : 0.0;
        if constexpr (DK) {
            const double p1 = lane_ssum(E * d1, lane), p2 = lane_ssum(E * d2, lane);
            o1 = valid ? vD * (k0cc * p1) : 0.0;
            o2 = valid ? vD * (k0cc * p2) : 0.0;
        } else {
            const double *b1 = scan_x(E * d1, true);
            const double *b2 = scan_x(E * d2, true);
            __syncthreads();
            o1 = valid ? vD * mix_trans(b1) : 0.0;
            o2 = valid ? vD * mix_trans(b2) : 0.0;
        }
    };
    // cross-wave max / sum of R per-lane values (uniform result in every thread)
    int rb = 0;
    auto block_reduce = [&](auto &v, unsigned sum_mask) {
        constexpr int R = sizeof(v) / sizeof(double);
#pragma unroll
        for (int i = 0; i < R; i++) v[i] = ((sum_mask >> i) & 1) ? wsum(v[i]) : wmax(v[i]);
        if (lane == 0)
#pragma unroll
            for (int i = 0; i < R; i++) s_red[rb][wv][i] = v[i];
        __syncthreads();
#pragma unroll
        for (int i = 0; i < R; i++) {
            const double *r = &s_red[rb][0][i];
            v[i] = ((sum_mask >> i) & 1) ? ((r[0] + r[16]) + (r[32] + r[48]))
                                         : fmax(fmax(r[0], r[16]), fmax(r[32], r[48]));
        }
        rb ^= 1;
    };
    int svr = 0, svw = 0;  // the rhs buffer the next GEMV reads / the next rhs goes to
    auto st_rhs = [&](double r) {
        vrhs = r;
        if (valid) s_vec[svw][seg_of(e)] = r;
        svr = svw;
        if (ONE) svw ^= 1;
    };
    auto make_rhs = [&]() {  // rhs = sigma x - q^ + A^'(rho z - y)
        const double d = (rho * vzt - vyt) - (rho * vzb - vyb);
        const double atw = At_of(valid ? d : 0.0);
        st_rhs(valid ? (sigma * vx - vqh) + atw : 0.0);
    };

    const int ct = st.check_termination;
    const int ai = (st.adaptive_rho && a.adaptive_interval) ? a.adaptive_interval : 0;
    int it = 0, nfact = 0;
    int next_check = ct ? ct : -1, next_adapt = ai ? ai : -1;

    auto finalize = [&]() {  // OSQP store_solution + the MPC front end's U += x[0:nu] (:105)
        const bool has_sol = status == kSolved || status == kSolvedInaccurate || status == kMaxIterReached;
        const bool keep = has_sol || status == kInvalidBounds || status == kTypeChanged;
        if (valid) {
            const double x = vx, zt = vzt, zb = vzb, yt = vyt, yb = vyb;
            const double D = vD, E = vE;
            const double xv = has_sol ? x * D : __builtin_nan("");
            // (the element index laundered here: hoisted out of the solve loop, the eight store addresses
            // were held across it and spilled to scratch, ~40 KB of writes per QP)
            const int eo = opaque(e);
            const size_t on = (size_t)b * n + eo, om = (size_t)b * m + eo;
            if (a.x) a.x[on] = xv;
            if (a.y) {
                const double cinv = cfg(7);
                a.y[om] = has_sol ? (yt * E) * cinv : __builtin_nan("");
                a.y[om + n] = has_sol ? (yb * E) * cinv : __builtin_nan("");
            }
            if (k == 0 && status == kSolved) a.U[(size_t)b * NU + c] = a.U[(size_t)b * NU + c] + xv;
            a.xs[on] = keep ? x : 0.0;
            a.zs[om] = keep ? zt : 0.0;
            a.zs[om + n] = keep ? zb : 0.0;
            a.ys[om] = keep ? yt : 0.0;
            a.ys[om + n] = keep ? yb : 0.0;
        }
        if (t == 0) {
            a.rhos[b] = rho;
            a.status[b] = status;
            a.iter[b] = it;
            a.rho_out[b] = rho;
        }
    };

    if (status != kUnsolved) {
        finalize();
        return;
    }
    make_rhs();  // (its barrier also orders the front end's LDS writes before every read below)

    int fail = 0;
    double Mb[4][16];
    // rows row_nat(i), columns 16 cg + j (P^ rows are padded to L.ldp: aligned, in-bounds loads);
    // the padding beyond n is the identity
    auto load_P = [&]() {
        const int seg = 16 * cg < L.ldp - 16 ? 16 * cg : L.ldp - 16;
        const int r = rg_here();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int gi = row_nat(r, i);
            const double2 *row = (const double2 *)(ops + L.Ph + (size_t)(gi < n ? gi : n - 1) * L.ldp + seg);
#pragma unroll
            for (int j = 0; j < 8; j++) {
                const double2 v = row[j];
                const int gj = 16 * cg + 2 * j;
                Mb[i][2 * j] = (gi < n && gj < n) ? v.x : (gi == gj ? 1.0 : 0.0);
                Mb[i][2 * j + 1] = (gi < n && gj + 1 < n) ? v.y : (gi == gj + 1 ? 1.0 : 0.0);
            }
#pragma unroll
            for (int j = 0; j < 16; j++) asm volatile("" : "+v"(Mb[i][j]));  // one row of loads in flight
        }
    };
    // + sigma I + r D SW[max(bi, bj)] D on the n x n part (block of row gi: row_blk(i))
    auto add_kkt = [&](double r) {
        double di[4];
        const int rl = rg_here();
#pragma unroll
        for (int i = 0; i < 4; i++) {
            const int bi = row_blk(rl, i);
            di[i] = s_D[row_cmp(rl, i) * 32 + (bi < 31 ? bi : 31)];
        }
#pragma unroll
        for (int jc = 0; jc < 4; jc++) {
#pragma unroll
            for (int jj = 0; jj < 4; jj++) {
                const int j = 4 * jc + jj, gj = 16 * cg + j;
                const int bj = (16 * cg) / NU + j / NU, cj = j % NU;
                const double dj = s_D[cj * 32 + (bj < 31 ? bj : 31)];
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    const int gi = row_nat(rl, i), bi = row_blk(rl, i), ci = row_cmp(rl, i);
                    const int bm = bi > bj ? bi : bj;
                    const double g = (di[i] * dj) * s_SW[(bm < 31 ? bm : 31) * 16 + ci * 4 + cj];
                    const double v = Mb[i][j] + (gi == gj ? sigma : 0.0) + r * g;
                    if (gi < n && gj < n) Mb[i][j] = v;
                }
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
#pragma unroll
                for (int jj = 0; jj < 4; jj++) asm volatile("" : "+v"(Mb[i][4 * jc + jj]));  // (as in invert)
        }
    };
    // part[i] = row row_nat(i) of M . in, in all 8 lanes of the row group (combined by DPP)
    auto gemv_rows = [&](const double *in, double (&part)[4]) {
        double s0[4], s1[4];
#pragma unroll
        for (int i = 0; i < 4; i++) s0[i] = s1[i] = 0.0;
        const double2 *v2 = (const double2 *)(in + kSegLd * cg);
        double2 q0 = v2[0], q1 = v2[1];
#pragma unroll
        for (int h = 0; h < 4; h++) {  // 4-column chunks (register budget), the next one in flight
            const double2 p0 = q0, p1 = q1;
            if (h < 3) {
                q0 = v2[2 * h + 2];
                q1 = v2[2 * h + 3];
            }
#pragma unroll
            for (int i = 0; i < 4; i++) {
                s0[i] = __builtin_fma(Mb[i][4 * h], p0.x, s0[i]);
                s1[i] = __builtin_fma(Mb[i][4 * h + 1], p0.y, s1[i]);
                s0[i] = __builtin_fma(Mb[i][4 * h + 2], p1.x, s0[i]);
                s1[i] = __builtin_fma(Mb[i][4 * h + 3], p1.y, s1[i]);
            }
#pragma unroll
            for (int i = 0; i < 4; i++) asm volatile("" : "+v"(s0[i]), "+v"(s1[i]));  // one chunk live at a time
        }
#pragma unroll
        for (int i = 0; i < 4; i++) {
            part[i] = s0[i] + s1[i];
            part[i] += dpp_t<0xB1>(part[i]);   // quad_perm [1,0,3,2]
            part[i] += dpp_t<0x4E>(part[i]);   // quad_perm [2,3,0,1]
            part[i] += dpp_t<0x141>(part[i]);  // row_half_mirror: the other quad of the 8
        }
    };
    // outv[component-major slot of row_nat(i)] = row row_nat(i) of M . in
    auto gemv = [&](const double *in, double *outv) {
        double part[4];
        gemv_rows(in, part);
        if (cg == 0)
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (row_nat(rg, i) < n) outv[row_cmp(rg, i) * 32 + row_blk(rg, i)] = part[i];
    };
    // ONE: this lane's element (block k, component c) of M . in, from lane 8 (k >> 2) + (k & 3) of the
    // same wave, whose register row (its cg & 3) is block k
    auto gemv_own = [&](const double *in) {
        double part[4];
        gemv_rows(in, part);
        const int ci = cg & 3;
        const double sel = ci == 0 ? part[0] : ci == 1 ? part[1] : ci == 2 ? part[2] : part[3];
        return __shfl(sel, 8 * ((k >> 2) & 7) + (k & 3), 64);
    };
    // Gauss-Jordan on pivot pairs K = {k, k + 1} (SPD: no pivoting; n odd pairs the last pivot with
    // the identity padding, which the update leaves as it is): A <- A - A(:,K) A_KK^-1 A(K,:) off K,
    // then rows K <- A_KK^-1 A(K,:), columns K <- -A(:,K) A_KK^-1, A_KK <- A_KK^-1.  One LDS broadcast of
    // the two rows and one barrier per pair; column K is read off the rows (the trailing block stays
    // symmetric, a_ik = a_ki, and the pivoted rows are its negation, a_ik = -a_ki: [A11^-1,
    // A11^-1 A12; -A21 A11^-1, S]).  k = 16 kb + kk with kk unrolled: the owner of column k is cg == kb
    // (register column kk), of row k rg == k >> 2 (register row kk & 3; ONE: rg == 8 (kk & 3) + kb,
    // register row kk >> 2).  Every thread forms A_KK^-1 from the broadcast (one division); the row
    // owners' rows restart from 0 and take the same FMA update with multipliers A_KK^-1.
    auto invert = [&]() {
        const int nkb = (n + 15) >> 4;
        for (int kb = 0; kb < nkb; kb++) {
#pragma unroll
            for (int kk = 0; kk < 16; kk += 2) {
                const int kp = 16 * kb + kk;
                if (kp >= n) continue;  // (not break: the loop must fully unroll, or Mb leaves the VGPRs)
                const int p = (kk >> 1) & 1;
                const int rk = ONE ? kk >> 2 : kk & 3, rl = ONE ? kk >> 2 : (kk & 3) + 1;
                const bool ownk = ONE ? rg == 8 * (kk & 3) + kb : rg == (kp >> 2);
                const bool ownl = ONE ? rg == 8 * (kk & 3) + 8 + kb : rg == (kp >> 2);
                const bool coln = cg == kb;
                if (ownk) {
                    double2 *r2 = (double2 *)&s_row[p][0][kSegLd * cg];
#pragma unroll
                    for (int j = 0; j < 8; j++) r2[j] = make_double2(Mb[rk][2 * j], Mb[rk][2 * j + 1]);
                }
                if (ownl) {
                    double2 *r2 = (double2 *)&s_row[p][1][kSegLd * cg];
#pragma unroll
                    for (int j = 0; j < 8; j++) r2[j] = make_double2(Mb[rl][2 * j], Mb[rl][2 * j + 1]);
                }
                __syncthreads();
                const double *R0 = s_row[p][0], *R1 = s_row[p][1];
                const double2 *k2 = (const double2 *)&R0[kSegLd * cg], *l2 = (const double2 *)&R1[kSegLd * cg];
                double2 qk = k2[0], ql = l2[0];  // row chunk 0, in flight with the pivot block
                const double2 pk = *(const double2 *)&R0[kSegLd * kb + kk];  // a_kk, a_kl
                const double all = R1[kSegLd * kb + kk + 1];
                const double det = __builtin_fma(pk.x, all, -(pk.y * pk.y));
                if (!(pk.x > 0.0) || !(det > 0.0)) fail = 1;
                const double idet = 1.0 / det;
                const double ikk = all * idet, ikl = -pk.y * idet, ill = pk.x * idet;
                double ck[4], cl[4];  // a_ik, a_il of this thread's rows, read off rows k, l
                if constexpr (ONE) {  // columns 16 (rg & 7) + 4 i + (rg >> 3)
                    const int r = rg_here();
                    const int o = kSegLd * (r & 7) + (r >> 3);
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        ck[i] = R0[o + 4 * i];
                        cl[i] = R1[o + 4 * i];
                    }
                } else {
                    const int o = kSegLd * (rg >> 2) + 4 * (rg & 3);
                    const double2 u0 = *(const double2 *)&R0[o], u1 = *(const double2 *)&R0[o + 2];
                    const double2 w0 = *(const double2 *)&R1[o], w1 = *(const double2 *)&R1[o + 2];
                    ck[0] = u0.x; ck[1] = u0.y; ck[2] = u1.x; ck[3] = u1.y;
                    cl[0] = w0.x; cl[1] = w0.y; cl[2] = w1.x; cl[3] = w1.y;
                }
                double fk[4], fl[4];  // -A(i,K) A_KK^-1 (rows K: A_KK^-1)
                {
                    const int r = rg_here();
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        const bool piv = row_nat(r, i) < kp;
                        const double a0 = piv ? -ck[i] : ck[i], a1 = piv ? -cl[i] : cl[i];
                        fk[i] = -__builtin_fma(a0, ikk, a1 * ikl);
                        fl[i] = -__builtin_fma(a0, ikl, a1 * ill);
                    }
                }
                if (ownk) {  // row k <- ikk a_k. + ikl a_l. (the row restarts from 0)
                    fk[rk] = ikk;
                    fl[rk] = ikl;
#pragma unroll
                    for (int j = 0; j < 16; j++) Mb[rk][j] = 0.0;
                }
                if (ownl) {  // row l <- ikl a_k. + ill a_l.
                    fk[rl] = ikl;
                    fl[rl] = ill;
#pragma unroll
                    for (int j = 0; j < 16; j++) Mb[rl][j] = 0.0;
                }
#pragma unroll
                for (int h = 0; h < 8; h++) {  // 2-column chunks of both rows, the next one in flight
                    double2 nk = qk, nl = ql;
                    if (h < 7) {
                        nk = k2[h + 1];
                        nl = l2[h + 1];
                    }
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        Mb[i][2 * h] = __builtin_fma(fk[i], qk.x, __builtin_fma(fl[i], ql.x, Mb[i][2 * h]));
                        Mb[i][2 * h + 1] = __builtin_fma(fk[i], qk.y, __builtin_fma(fl[i], ql.y, Mb[i][2 * h + 1]));
                    }
                    qk = nk;
                    ql = nl;
                    // pin the updates here: sunk below the fix-up branches they would keep every
                    // chunk of the rows live (register budget)
#pragma unroll
                    for (int i = 0; i < 4; i++) asm volatile("" : "+v"(Mb[i][2 * h]), "+v"(Mb[i][2 * h + 1]));
                }
                if (coln) {  // columns K: -A(i,K) A_KK^-1, rows K: A_KK^-1
#pragma unroll
                    for (int i = 0; i < 4; i++) {
                        Mb[i][kk] = fk[i];
                        Mb[i][kk + 1] = fl[i];
                    }
                    if (ownk) {
                        Mb[rk][kk] = ikk;
                        Mb[rk][kk + 1] = ikl;
                    }
                    if (ownl) {
                        Mb[rl][kk] = ikl;
                        Mb[rl][kk + 1] = ill;
                    }
                }
            }
        }
    };

    load_P();
    bool refactor = true, loaded = true, px_pending = load;
    for (;;) {
        if (refactor) {  // (re-)invert M(rho); the first factorisation also forms P^ x of a warm start
            if (!loaded) load_P();
            loaded = false;
            if (px_pending) {
                gemv(s_nat, s_out);
                __syncthreads();
                if (valid) vpx = s_out[vi];
                __syncthreads();  // s_out is the GEMV output below
                px_pending = false;
            }
            add_kkt(rho);
            invert();  // its first barrier orders the rhs writes before the GEMV below
            nfact++;
#ifndef MPCQ_GJ_STAMPS
            MPCQ_MSTAMP(2, __builtin_amdgcn_s_memtime());
#endif
            if (fail) {  // P^ + sigma I + rho A^'A^ not positive definite
                status = kNonCvx;
                finalize();
                break;
            }
            refactor = false;
        }
        double xt;
        if constexpr (ONE) {
            xt = gemv_own(s_vec[svr]);
        } else {
            gemv(s_vec[svr], s_out);
            __syncthreads();  // x~ ready
            xt = s_out[vi];
        }
        xt = valid ? xt : 0.0;
        it++;
        const bool at_check = it == next_check, at_adapt = it == next_adapt;
        if (at_check) next_check += ct;
        if (at_adapt) next_adapt += ai;
        const bool last = it == st.max_iter;
        const bool info = at_check || at_adapt || last;
        const double rinv = 1.0 / rho;
        // ---- x~ = M^-1 rhs ; z~ = A^ x~ ; P^ x~ = rhs - sigma x~ - rho A^'z~ ; relax ; project ; dual
        const double ztl = A_of(xt);
        double d2, dr, xn;
        {
            const double x = vx;
            xn = __builtin_fma(alpha, xt, oma * x);
            double zt = vzt, zb = vzb, yt = vyt, yb = vyb;
            const double ut = vut, ub = vub;
            // top row e and bottom row n + e (z~_bot = -z~_top)
            const double vt = __builtin_fma(alpha, ztl, oma * zt);
            const double zn_t = fmin(__builtin_fma(rinv, yt, vt), ut);
            const double dyt = rho * (vt - zn_t);
            yt = __builtin_fma(rho, vt - zn_t, yt);
            zt = zn_t;
            const double vb = __builtin_fma(alpha, -ztl, oma * zb);
            const double zn_b = fmin(__builtin_fma(rinv, yb, vb), ub);
            const double dyb = rho * (vb - zn_b);
            yb = __builtin_fma(rho, vb - zn_b, yb);
            zb = zn_b;
            d2 = 2.0 * ztl;
            dr = (rho * zt - yt) - (rho * zb - yb);  // next rhs (rho unchanged)
            {
                vx = valid ? xn : 0.0;
                vdx = valid ? xn - x : 0.0;
                vzt = valid ? zt : 0.0; vzb = valid ? zb : 0.0;
                vyt = valid ? yt : 0.0; vyb = valid ? yb : 0.0;
                vdyt = valid ? dyt : 0.0; vdyb = valid ? dyb : 0.0;
            }
        }
        double gz, atw = 0.0;
        if (info)
            gz = At_of(valid ? d2 : 0.0);
        else
            At_of2(valid ? d2 : 0.0, valid ? dr : 0.0, gz, atw);
        {  // carried P^ x (KKT identity)
            const double px = vpx;
            const double ptx = (vrhs - sigma * xt) - rho * gz;
            const double pxn = __builtin_fma(alpha, ptx, oma * px);
            {
                vpx = valid ? pxn : 0.0;
                vdpx = valid ? pxn - px : 0.0;
            }
        }
        int ctl = 0;  // 0 continue, 1 refactor, 2 done
        if (info) {
            // ---- update_info: residuals (scaled norms _r, unscaled _s as OSQP reports them)
            // OSQP's tests read ||z||, ||A x|| only as max(||z||, ||A x||) and ||q||, ||A' y||, ||P x|| only as
            // their maximum: one reduction of the lanes' maxima each (max is exact in any order), eight
            // values per check instead of fourteen
            double v[8];
            {
                const double ax = A_of(valid ? vx : 0.0);
                const double zt = vzt, zb = vzb, ei = 1.0 / vE;
                const double rt = ax - zt, rbm = -ax - zb;
                v[0] = fmax(fabs(rt), fabs(rbm));                                  // ax_z
                v[1] = fmax(fabs(ei * rt), fabs(ei * rbm));                        // ax_zs
                v[2] = fmax(fmax(fabs(zt), fabs(zb)), fabs(ax));                   // max(zn_r, axn_r)
                v[3] = fmax(fmax(fabs(ei * zt), fabs(ei * zb)), fabs(ei * ax));    // max(zn_s, axn_s)
            }
            {
                const double aty = At_of(valid ? vyt - vyb : 0.0);
                const double qh = vqh, px = vpx, di = 1.0 / vD;
                const double r = (qh + px) + aty;
                v[4] = fabs(r);                                                    // dr_r
                v[5] = fabs(di * r);                                               // dr_s
                v[6] = fmax(fmax(fabs(qh), fabs(aty)), fabs(px));                  // max(qn_r, atyn_r, pxn_r)
                v[7] = fmax(fmax(fabs(di * qh), fabs(di * aty)), fabs(di * px));   // max(qn_s, atyn_s, pxn_s)
            }
            if (!valid)
#pragma unroll
                for (int i = 0; i < 8; i++) v[i] = 0.0;
            block_reduce(v, 0u);
            const double ax_z = v[0], ax_zs = v[1], zax_r = v[2], zax_s = v[3];
            const double dr_r = v[4], dr_s = v[5], qap_r = v[6], qap_s = v[7];
            const double cinv = cfg(7);
            const bool scaled_term = cfg(5) != 0.0;
            const double pri_res = scaled_term ? ax_z : ax_zs;
            const double dua_res = scaled_term ? dr_r : cinv * dr_s;

            // OSQP is_primal_infeasible on delta_y (u finite, l = -inf on every row: d = max(d, 0))
            auto primal_inf = [&](double eps) -> bool {
                const double dt_ = valid ? fmax(vdyt, 0.0) : 0.0, db_ = valid ? fmax(vdyb, 0.0) : 0.0;
                const double E = vE;
                double w[2];
                w[0] = fmax(fabs(scaled_term ? dt_ : E * dt_), fabs(scaled_term ? db_ : E * db_));  // ndy
                w[1] = valid ? vut * dt_ + vub * db_ : 0.0;                            // lhs
                block_reduce(w, 2u);
                const double ndy = w[0], lhs = w[1];
                if (!(ndy > kDivisionTol && lhs < eps * ndy)) return false;
                const double atd = At_of(dt_ - db_);
                double u[1] = {valid ? fabs(scaled_term ? atd : atd / vD) : 0.0};
                block_reduce(u, 0u);
                return u[0] < eps * ndy;
            };
            // OSQP is_dual_infeasible on delta_x (P^ delta_x = delta of the carried P^ x)
            auto dual_inf = [&](double eps) -> bool {
                const double dx = valid ? vdx : 0.0, D = vD;
                double w[3];
                w[0] = valid ? vqh * dx : 0.0;                                          // qdx
                w[1] = fabs(scaled_term ? dx : D * dx);                                      // ndx
                w[2] = valid ? fabs(scaled_term ? vdpx : vdpx / D) : 0.0;          // |P^ dx|
                block_reduce(w, 1u);
                const double qdx = w[0], ndx = w[1], npdx = w[2];
                const double cs = scaled_term ? 1.0 : cfg(6);
                if (!(qdx < 0.0 && ndx > kDivisionTol && qdx < -cs * eps * ndx)) return false;
                if (!(npdx < cs * eps * ndx)) return false;
                const double adx = A_of(dx);
                double u[1] = {0.0};
                if (valid) {
                    const double sv = scaled_term ? adx : adx / vE;
                    if (vut < kInfty * kMinScaling && sv > eps * ndx) u[0] = 1.0;   // top row
                    if (vub < kInfty * kMinScaling && -sv > eps * ndx) u[0] = 1.0;  // bottom row
                }
                block_reduce(u, 0u);
                return u[0] == 0.0;
            };
            auto check = [&](bool approx) -> int {
                const double mul = approx ? 10.0 : 1.0;
                const double ea = cfg(0) * mul, er = cfg(1) * mul;
                if (pri_res > kInfty || dua_res > kInfty) return kNonCvx;
                const double ep = ea + er * (scaled_term ? zax_r : zax_s);
                const double ed = ea + er * (scaled_term ? qap_r : cinv * qap_s);
                const bool pok = pri_res < ep, dok = dua_res < ed;
                if (pok && dok) return approx ? kSolvedInaccurate : kSolved;
                if (!pok && primal_inf(cfg(2) * mul))
                    return approx ? kPrimalInfeasibleInaccurate : kPrimalInfeasible;
                if (!dok && dual_inf(cfg(3) * mul))
                    return approx ? kDualInfeasibleInaccurate : kDualInfeasible;
                return kUnsolved;
            };
            // OSQP order: check at check iterations, adapt_rho at adapt iterations, and after the last
            // iteration an exact then an approximate check (osqp_solve); one call site for check()
            for (int pass = 0; pass < 2; pass++) {
                if (status != kUnsolved) break;
                if (pass == 0) {
                    if (at_check || last) status = check(false);
                    if (status == kUnsolved && at_adapt && !last) {  // adapt_rho (scaled norms)
                        const double pr = ax_z / (zax_r + kDivisionTol);
                        const double dn = qap_r;
                        const double du = dr_r / (dn + kDivisionTol);
                        double rn = rho * sqrt(pr / (du + kDivisionTol));
                        rn = fmin(fmax(rn, kRhoMin), kRhoMax);
                        if (rn > rho * cfg(4) || rn < rho / cfg(4)) {
                            rho = fmin(fmax(rn, kRhoMin), kRhoMax);
                            ctl = 1;
                        }
                    }
                } else if (last) {
                    const int s2 = check(true);
                    status = s2 != kUnsolved ? s2 : kMaxIterReached;
                }
            }
        }
        if (status != kUnsolved) {
            __syncthreads();  // every lane's state is final
            finalize();
            break;
        }
        if (info)
            make_rhs();  // rho may have changed
        else
            st_rhs(valid ? (sigma * xn - vqh) + atw : 0.0);
        refactor = ctl == 1;
        __syncthreads();  // next rhs ready
    }
#ifndef MPCQ_GJ_STAMPS
    if (a.stamps && t == 0) {
        a.stamps[(size_t)blockIdx.x * 8 + 3] = (long long)__builtin_amdgcn_s_memtime();
        a.stamps[(size_t)blockIdx.x * 8 + 4] = it;
        a.stamps[(size_t)blockIdx.x * 8 + 5] = nfact;
    }
#endif
