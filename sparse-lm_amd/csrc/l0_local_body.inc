// The ONE body of the l0 local search's kernels, included where a kernel's braces open (l0_local_kernels.hpp: l0_local_kernel<CARD>
// and l0_local_l1_kernel; the unit's head describes it).  It is a text and not a function: a body inlined into a thin kernel
// compiles to other code than the kernel it was (34 accumulation registers more in either older kernel, measured), and the
// older kernels must stay the code they were.  The including kernel provides
//     a      its argument (L0LsArgs, or L0LsL1Args)
//     CARD   constexpr bool: the cardinality rule (at the loop); else the penalised rule
//     L1     constexpr bool: the penalised rule with an l1 term -- the cell brings lam = l1s[e], lam ||beta||_1 joins F and the
//            coordinate of the descent and of both gains of the swap scan is l0_ls_coord_l1; never with CARD
//     l1s    const double*: the cells' l1 weights (read under L1 alone)
// What a rule does not use is compiled out (if constexpr).
  static_assert(!(CARD && L1), "best subset with an l1 term is no estimator of the reference");
  const int lane = threadIdx.x & 63;
  const int p = a.p, ns = (p + 63) >> 6;
  const long long ld = a.ld;
  const double big_M = a.big_M;
  const int stride = (int)gridDim.x * L0_WAVES;
  for (int q = (int)blockIdx.x * L0_WAVES + (int)(threadIdx.x >> 6); q < a.n_problems; q += stride) {
    const int rc = q / a.n_starts;                                  // r * n_cells + e
    const int rs = __builtin_amdgcn_readfirstlane(rc / a.n_cells);  // the row set: one per wave, so a scalar
    const int cell = rc - rs * a.n_cells;
    const double* __restrict__ G = a.G[rs];
    const double* __restrict__ cv = a.c[rs];
    const double tol = L0_CD_TOL * sqrt(a.yy[rs]);
    const double alpha = CARD ? 0.0 : a.alphas[cell], eta2 = 2.0 * a.etas[cell];
    double lam = 0.0;
    if constexpr (L1) lam = l1s[cell];
    double beta[L0_LS_SLOTS], r[L0_LS_SLOTS], d[L0_LS_SLOTS];
    double dmax = 0.0;
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s) {
      const int j = s * 64 + lane;
      beta[s] = 0.0;
      r[s] = 0.0;
      d[s] = 0.0;
      if (s < ns && j < p) {
        d[s] = G[(long long)j * ld + j] + eta2;
        r[s] = cv[j];
        if (a.starts) beta[s] = a.starts[(long long)q * p + j];
      }
      dmax = fmax(dmax, d[s]);
    }
    dmax = l0_wave_max(dmax);
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (!(d[s] > L0_PIVOT * dmax)) {  // d = 0 marks a column that stays out (and the lanes beyond p)
        d[s] = 0.0;
        beta[s] = 0.0;
      }
    // r = c - H beta of the start, column by column in ascending order
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (s < ns) {
        unsigned long long act = __ballot(beta[s] != 0.0);
        while (act) {
          const int k = __builtin_ctzll(act);
          act &= act - 1;
          l0_ls_axpy(r, G, ld, p, ns, lane, eta2, s * 64 + k, -l0_bcast(beta[s], k));
        }
      }

    int sweeps = 0, swaps = 0, status = 0;
    int kmax = 0, nact = 0, grows = 0, drops = 0;  // (the cardinality rule's: the cell's size, the support's, the two counts)
    if constexpr (CARD) {
      kmax = a.sizes[cell];
#pragma unroll
      for (int s = 0; s < L0_LS_SLOTS; ++s)
        if (s < ns) nact += __popcll(__ballot(beta[s] != 0.0));
      // ---- shrink: while the support is larger than k its weakest column leaves (only a start can be: nothing below adds beyond k)
      while (nact > kmax) {
        double gb = HUGE_VAL;
        int ib = 0x7fffffff;
#pragma unroll
        for (int t = 0; t < L0_LS_SLOTS; ++t)
          if (t < ns) {
            const double g = l0_ls_coord(r[t] + d[t] * beta[t], d[t], big_M).gain;
            if (beta[t] != 0.0 && g < gb) {  // (ascending slots: the lane keeps its lowest i on ties)
              gb = g;
              ib = t * 64 + lane;
            }
          }
        const double gmin = -l0_wave_max(-gb);
        const int imin = l0_ls_wave_min(gb == gmin ? ib : 0x7fffffff);
        if (imin == 0x7fffffff) break;
        double mine = 0.0;
#pragma unroll
        for (int t = 0; t < L0_LS_SLOTS; ++t)
          if (t == (imin >> 6)) {
            mine = beta[t];
            if (lane == (imin & 63)) beta[t] = 0.0;
          }
        l0_ls_axpy(r, G, ld, p, ns, lane, eta2, imin, l0_bcast(mine, imin & 63));
        --nact;
        ++drops;
      }
    }
    for (;;) {
      // ---- 1. the descent to its fixed point (the cardinality rule: on the support alone, no threshold, b == 0 leaves) ---------
      for (int sw = 0;; ++sw) {
        if (sw == L0_CD_SWEEPS) {
          status |= L0_LS_SWEEPS_OUT;
          break;
        }
        bool moved = false;
        double maxd = 0.0;
        int cursor = 0;
        for (;;) {  // the next change at or after the cursor
          const int s0 = cursor >> 6;
          bool found = false;
          int jf = 0;
          double delta = 0.0;
#pragma unroll
          for (int s = 0; s < L0_LS_SLOTS; ++s)
            if (!found && s >= s0 && s < ns) {
              const L0LsCoord cd = l0_ls_coord_of<L1>(r[s] + d[s] * beta[s], d[s], big_M, lam);
              const double nb = CARD ? cd.b : l0_ls_threshold(cd, alpha);
              const unsigned long long bal = __ballot((CARD ? beta[s] != 0.0 : d[s] > 0.0) && s * 64 + lane >= cursor && nb != beta[s]);
              if (bal) {
                const int k = __builtin_ctzll(bal);
                const double nbk = l0_bcast(nb, k), old = l0_bcast(beta[s], k), dk = l0_bcast(d[s], k);
                if (lane == k) beta[s] = nbk;
                found = true;
                jf = s * 64 + k;
                delta = nbk - old;
                moved = moved || ((nbk != 0.0) != (old != 0.0));
                if constexpr (CARD)
                  if (nbk == 0.0) {
                    --nact;
                    ++drops;
                  }
                maxd = fmax(maxd, fabs(delta) * sqrt(dk));
              }
            }
          if (!found) break;
          l0_ls_axpy(r, G, ld, p, ns, lane, eta2, jf, -delta);
          cursor = jf + 1;
        }
        ++sweeps;
        if (!moved && maxd <= tol) break;
      }
      if constexpr (CARD) {
        // ---- grow: below k, the outside column with the largest gain enters -- if it would move by more than the descent's own
        // stopping tolerance -- and the descent runs again.  The swap scan's arg-max without a removed column and without a row read.
        if (status) break;
        if (nact < kmax) {
          double gb = -1.0, bb = 0.0;
          int jb = 0x7fffffff;
#pragma unroll
          for (int t = 0; t < L0_LS_SLOTS; ++t)
            if (t < ns) {
              const L0LsCoord co = l0_ls_coord(r[t], d[t], big_M);
              if (d[t] > 0.0 && beta[t] == 0.0 && co.gain > gb) {  // (ascending slots: the lane keeps its lowest j on ties)
                gb = co.gain;
                bb = fabs(co.b) * sqrt(d[t]) > tol ? co.b : 0.0;  // (0: it would not move)
                jb = t * 64 + lane;
              }
            }
          const double gmax = l0_wave_max(gb);
          const int jmin = l0_ls_wave_min(gb == gmax ? jb : 0x7fffffff);
          const double bj = jmin != 0x7fffffff ? l0_bcast(bb, jmin & 63) : 0.0;  // (that lane's best IS jmin)
          if (bj != 0.0) {
#pragma unroll
            for (int t = 0; t < L0_LS_SLOTS; ++t)
              if (t == (jmin >> 6) && lane == (jmin & 63)) beta[t] = bj;
            l0_ls_axpy(r, G, ld, p, ns, lane, eta2, jmin, -bj);
            ++nact;
            ++grows;
            continue;
          }
        }
      }
      if (!a.swaps || status) break;
      // ---- 2. the swap scan: the first i of the support that a column outside replaces with a gain ----------------------------
      bool swapped = false;
#pragma unroll
      for (int si = 0; si < L0_LS_SLOTS; ++si)
        if (!swapped && si < ns) {
          unsigned long long act = __ballot(beta[si] != 0.0);
          while (act && !swapped) {
            const int k = __builtin_ctzll(act);
            act &= act - 1;
            const int i = si * 64 + k;
            const double bi = l0_bcast(beta[si], k), di = l0_bcast(d[si], k), ri = l0_bcast(r[si], k);
            const double gi = l0_ls_coord_of<L1>(ri + di * bi, di, big_M, lam).gain;
            const double* row = G + (long long)i * ld;
            double gb = -1.0, bb = 0.0;
            int jb = 0x7fffffff;
#pragma unroll
            for (int t = 0; t < L0_LS_SLOTS; ++t)
              if (t < ns) {
                const int j = t * 64 + lane;
                const double h = j < p ? row[j] : 0.0;
                const L0LsCoord co = l0_ls_coord_of<L1>(r[t] + h * bi, d[t], big_M, lam);
                if (d[t] > 0.0 && beta[t] == 0.0 && co.gain > gb) {  // (ascending slots: the lane keeps its lowest j on ties)
                  gb = co.gain;
                  bb = co.b;
                  jb = j;
                }
              }
            const double gmax = l0_wave_max(gb);
            const int jmin = l0_ls_wave_min(gb == gmax ? jb : 0x7fffffff);
            if (jmin != 0x7fffffff && l0_ls_swap_better(gmax, gi, alpha)) {
              const double bj = l0_bcast(bb, jmin & 63);  // (that lane's best IS jmin)
              if (lane == k) beta[si] = 0.0;
              l0_ls_axpy(r, G, ld, p, ns, lane, eta2, i, bi);
#pragma unroll
              for (int t = 0; t < L0_LS_SLOTS; ++t)
                if (t == (jmin >> 6) && lane == (jmin & 63)) beta[t] = bj;
              l0_ls_axpy(r, G, ld, p, ns, lane, eta2, jmin, -bj);
              ++swaps;
              swapped = true;
            }
          }
        }
      if (!swapped) break;
      if (swaps == L0_LS_SWAPS) {
        status |= L0_LS_SWAPS_OUT;
        break;
      }
    }

    // F = 1/2 beta^T H beta - c^T beta (+ lam ||beta||_1) + alpha nnz with H beta = c - r; the problem's own row of every output
    double acc = 0.0, l1 = 0.0;
    int nnz = 0;
#pragma unroll
    for (int s = 0; s < L0_LS_SLOTS; ++s)
      if (s < ns) {
        const int j = s * 64 + lane;
        if (j < p) {
          acc += beta[s] * (cv[j] + r[s]);
          if constexpr (L1) l1 += fabs(beta[s]);
          nnz += beta[s] != 0.0;
          a.beta_out[(long long)q * p + j] = beta[s];
        }
      }
    acc = l0_wave_sum(acc);
    if constexpr (L1) l1 = l0_wave_sum(l1);
    nnz = (int)l0_wave_sum((double)nnz);
    if (lane == 0) {
      if constexpr (L1)
        a.F_out[q] = -0.5 * acc + lam * l1 + alpha * (double)nnz;
      else
        a.F_out[q] = -0.5 * acc + alpha * (double)nnz;
      int* stat = a.stat_out + (long long)q * a.stat_stride;
      stat[0] = sweeps;
      stat[1] = swaps;
      stat[2] = status;
      stat[3] = nnz;
      if constexpr (CARD) {
        stat[4] = grows;
        stat[5] = drops;
      }
    }
  }
