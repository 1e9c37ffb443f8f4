// TEST INFRASTRUCTURE: the articulated step with the per-slot contact impulse report the GPU kernels of mh_artic_rp.hip are held to
// (include/moby_hip_artic.h, "Contact report").
//
// tests/native/artic_boxsphere_ref.cpp is included as it stands (its helpers are file-local and existing files are not edited for a feature); its
// step / do_mini_step / handle_impacts2 are restated below with three additions: an accumulator per contact that every apply() adds to (the
// reference's contact_impulse, ImpactConstraintHandler.cpp:298-327), the fold of a mini-step's contacts into the step's rows after the handler
// returned without a throw (where ConstraintSimulator::constraint_post_callback_fn sees them, CSim:353), and a sink pointer that may be NULL.
// Everything else is that file's text.  Pins (tests/test_artic_report.py): with and without a sink it equals artic_boxsphere_ref_step bit for bit.
// Built by the tests with g++ and oracle/Makefile's CXXFLAGS (-ffp-contract=off), linked with artic_box_ref.cpp, artic_drive_ref.cpp,
// artic_pose_ref.cpp and artic_pair_ref.cpp, as a library of its own.
#include "artic_boxsphere_ref.cpp"

namespace {

constexpr int RP = MH_REPORT_PAIR;

struct ArticR : ArticP {
  using ArticP::ArticP;
  // what the tests ask of a scene, per step: the mini-steps that were folded, and the normal impulses of every handler call's FIRST application (a
  // row whose [1] exceeds their sum has seen a restitution pass or a second solve)
  int folds = 0; double first_cn = 0.0;

  // ArticP::handle_impacts2 with acc: 3 doubles per contact, (cn, cs, ct) accumulated over every application of impulses; zero on entry
  void handle_impacts_r(const std::vector<PC>& cs, std::vector<double>& acc) {
    using namespace artic;
    const int nc = (int)cs.size();
    int idx[2 * NJ]; bool upper[2 * NJ]; int nl = 0;
    for (int i = 0; i < nj; i++) {                                   // ArticulatedBody.inl:9-43 (q_tare = 0)
      if (q[i] >= m->hilimit[i]) { idx[nl] = i; upper[nl] = true; nl++; }
      if (q[i] <= m->lolimit[i]) { idx[nl] = i; upper[nl] = false; nl++; }
    }
    if (nc + nl == 0) return;
    double V[NJ][6]; link_velocities(V);
    bool impacting = false;                                          // CSim:313-323
    for (int i = 0; i < nc; i++) if (cvel(V, cs[i]) < -A_NEAR_ZERO) impacting = true;
    for (int k = 0; k < nl; k++) { const double v = upper[k] ? -qd[idx[k]] : qd[idx[k]]; if (v < -A_NEAR_ZERO) impacting = true; }
    if (!impacting) return;
    const bool noslip = (nc == 0) || (m->cp_mu_coulomb >= 1e2);
    const int n = nc + nl;
    const int nk = (m->cp_nk > 0) ? m->cp_nk : 4, kh = nk / 2;
    const int nvars = 5 * nc + nl, N = nvars + nc + nl + nc * kh;    // ICH-QP:97-112
    if (noslip ? (n > MH_NOSLIP_MAX) : (N > MH_LCP_MAX_N_WAVE || nl > MH_NOSLIP_MAX)) { aux->status |= MH_WORLD_UNSUPPORTED; return; }
    if (m->algorithm == MH_ARTIC_FSAB) crba();                       // get_generalized_inertia (ICH:1600-1607)
    std::vector<double> X(H, H + nj * nj);
    if (!inverse_spd(nj, X.data(), nj)) { aux->status |= MH_WORLD_LCP_FAILED; return; }
    std::vector<double> C[3], XC[3];                                 // C[d]: nc x nj; XC[d] = C[d] X (rows of X_CdT')
    for (int d = 0; d < 3; d++) { C[d].assign((size_t)nc * nj, 0.0); XC[d].assign((size_t)nc * nj, 0.0); }
    for (int i = 0; i < nc; i++) {
      const double* dirs[3] = { cs[i].n, cs[i].sv, cs[i].tv };
      for (int d = 0; d < 3; d++) for (int j = 0; j < nj; j++) C[d][(size_t)i * nj + j] = contact_row(cs[i], j, dirs[d]);
    }
    for (int d = 0; d < 3; d++) for (int i = 0; i < nc; i++) for (int c = 0; c < nj; c++) {
      double a = 0.0; for (int k = 0; k < nj; k++) a = a + C[d][(size_t)i * nj + k] * X[k * nj + c];
      XC[d][(size_t)i * nj + c] = a;
    }
    std::vector<double> G[3][3], CL[3], Cv[3];
    for (int a = 0; a < 3; a++) for (int b = a; b < 3; b++) {
      G[a][b].assign((size_t)nc * nc, 0.0);
      for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j++) { double s = 0.0; for (int k = 0; k < nj; k++) s = s + C[a][(size_t)i * nj + k] * XC[b][(size_t)j * nj + k]; G[a][b][(size_t)i * nc + j] = s; }
    }
    for (int d = 0; d < 3; d++) {
      CL[d].assign((size_t)nc * (nl > 0 ? nl : 1), 0.0); Cv[d].assign(nc, 0.0);
      for (int i = 0; i < nc; i++) {
        for (int k2 = 0; k2 < nl; k2++) { double s = 0.0; for (int k = 0; k < nj; k++) s = s + C[d][(size_t)i * nj + k] * X[idx[k2] * nj + k]; CL[d][(size_t)i * nl + k2] = s; }
        double s = 0.0; for (int k = 0; k < nj; k++) s = s + C[d][(size_t)i * nj + k] * qd[k];
        Cv[d][i] = s;
      }
    }
    std::vector<double> LL((size_t)nl * nl + 1), Lv(nl + 1);
    for (int a = 0; a < nl; a++) for (int b = a; b < nl; b++) { const double e = X[idx[a] * nj + idx[b]]; LL[a + (size_t)nl * b] = e; LL[b + (size_t)nl * a] = e; }
    for (int k = 0; k < nl; k++) { Lv[k] = qd[idx[k]]; if (upper[k]) Lv[k] = -Lv[k]; }

    std::vector<double> cn(nc, 0.0), csv(nc, 0.0), ctv(nc, 0.0), l(nl, 0.0);
    int applications = 0;
    // dv = X_CnT cn + X_CsT cs + X_CtT ct + X_LT sl (ICH:1365-1373, 345-352); the report: contact_impulse += what was applied
    auto apply = [&]() {
      std::vector<double> dv(nj, 0.0), t(nj);
      const std::vector<double>* imp[3] = { &cn, &csv, &ctv };
      for (int d = 0; d < 3; d++) {
        for (int r = 0; r < nj; r++) { double s = 0.0; for (int i = 0; i < nc; i++) s = s + XC[d][(size_t)i * nj + r] * (*imp[d])[i]; t[r] = s; }
        for (int r = 0; r < nj; r++) dv[r] = (d == 0) ? t[r] : dv[r] + t[r];
      }
      for (int r = 0; r < nj; r++) { double s = 0.0; for (int k = 0; k < nl; k++) { const double ls = upper[k] ? -l[k] : l[k]; s = s + ls * X[idx[k] * nj + r]; } t[r] = s; }
      for (int r = 0; r < nj; r++) dv[r] = dv[r] + t[r];
      for (int r = 0; r < nj; r++) qd[r] = qd[r] + dv[r];
      for (int i = 0; i < nc; i++) { acc[3*i] = acc[3*i] + cn[i]; acc[3*i + 1] = acc[3*i + 1] + csv[i]; acc[3*i + 2] = acc[3*i + 2] + ctv[i]; }
      if (applications++ == 0) for (int i = 0; i < nc; i++) first_cn = first_cn + cn[i];
    };
    auto Gs = [&](int a, int b, int i, int j) -> double { return (a <= b) ? G[a][b][(size_t)i * nc + j] : G[b][a][(size_t)j * nc + i]; };
    auto update_vels = [&]() {                                       // update_constraint_velocities_from_impulses (ICH:427-464)
      const std::vector<double>* imp[3] = { &cn, &csv, &ctv };
      for (int a = 0; a < 3; a++) {
        for (int b = 0; b < 3; b++) {
          std::vector<double> t(nc, 0.0);
          for (int i = 0; i < nc; i++) { double s = 0.0; for (int j = 0; j < nc; j++) s = s + Gs(a, b, i, j) * (*imp[b])[j]; t[i] = s; }
          for (int i = 0; i < nc; i++) Cv[a][i] = Cv[a][i] + t[i];
        }
        for (int i = 0; i < nc; i++) { double s = 0.0; for (int k = 0; k < nl; k++) s = s + CL[a][(size_t)i * nl + k] * l[k]; Cv[a][i] = Cv[a][i] + s; }
      }
      for (int d = 0; d < 3; d++) for (int k = 0; k < nl; k++) { double s = 0.0; for (int i = 0; i < nc; i++) s = s + CL[d][(size_t)i * nl + k] * (*imp[d])[i]; Lv[k] = Lv[k] + s; }
      std::vector<double> t(nl + 1, 0.0);
      for (int r = 0; r < nl; r++) { double s = 0.0; for (int k = 0; k < nl; k++) s = s + LL[r + (size_t)nl * k] * l[k]; t[r] = s; }
      for (int r = 0; r < nl; r++) Lv[r] = Lv[r] + t[r];
    };
    auto minv_of = [&]() {                                           // calc_min_constraint_velocity (ICH:413-424)
      double mn = A_INF;
      for (int i = 0; i < nc; i++) mn = (i == 0 || Cv[0][i] < mn) ? Cv[0][i] : mn;
      if (nl > 0) { double ml = Lv[0]; for (int k = 1; k < nl; k++) ml = (Lv[k] < ml) ? Lv[k] : ml; mn = (ml < mn) ? ml : mn; }
      return mn;
    };
    auto solve_noslip = [&]() -> bool {                              // apply_no_slip_model (ICH:1009-1417)
      std::vector<int> Sx, Tx; std::vector<double> Y;
      auto build_Y = [&](bool skew) -> int {
        const int ns = (int)Sx.size(), nt = (int)Tx.size(), mm = ns + nt;
        Y.assign((size_t)mm * mm + 1, 0.0);
        for (int a = 0; a < ns; a++) for (int b = 0; b < ns; b++) Y[a + (size_t)mm * b] = G[1][1][(size_t)Sx[a] * nc + Sx[b]];
        for (int a = 0; a < nt; a++) for (int b = 0; b < nt; b++) Y[(ns + a) + (size_t)mm * (ns + b)] = G[2][2][(size_t)Tx[a] * nc + Tx[b]];
        for (int a = 0; a < ns; a++) for (int b = 0; b < nt; b++) { const double g = G[1][2][(size_t)Sx[a] * nc + Tx[b]]; Y[a + (size_t)mm * (ns + b)] = g; Y[(ns + b) + (size_t)mm * a] = g; }
        if (skew) for (int j = 0; j < mm; j++) Y[j + (size_t)mm * j] = Y[j + (size_t)mm * j] - A_NEAR_ZERO;
        return mm;
      };
      for (int i = 0; i < nc; i++) {                                 // greedy largest non-singular tangent set (ICH:1087-1145)
        Sx.push_back(i); int mm = build_Y(true); if (!chol_factor(mm, Y.data(), mm)) Sx.pop_back();
        Tx.push_back(i); mm = build_Y(true);     if (!chol_factor(mm, Y.data(), mm)) Tx.pop_back();
      }
      const int ns = (int)Sx.size(), nt = (int)Tx.size();
      const int mm = build_Y(false);
      if (mm > 0 && !chol_factor(mm, Y.data(), mm)) { aux->status |= MH_WORLD_LCP_FAILED; return false; }   // assert(success)
      std::vector<double> QX((size_t)n * mm + 1);
      for (int i = 0; i < nc; i++) {
        for (int a = 0; a < ns; a++) QX[(size_t)i * mm + a] = G[0][1][(size_t)i * nc + Sx[a]];
        for (int a = 0; a < nt; a++) QX[(size_t)i * mm + ns + a] = G[0][2][(size_t)i * nc + Tx[a]];
      }
      for (int k = 0; k < nl; k++) {
        for (int a = 0; a < ns; a++) QX[(size_t)(nc + k) * mm + a] = CL[1][(size_t)Sx[a] * nl + k];
        for (int a = 0; a < nt; a++) QX[(size_t)(nc + k) * mm + ns + a] = CL[2][(size_t)Tx[a] * nl + k];
      }
      std::vector<double> W((size_t)mm * n + 1), col(mm + 1);
      for (int j = 0; j < n; j++) {
        for (int a = 0; a < mm; a++) col[a] = QX[(size_t)j * mm + a];
        if (mm > 0) chol_solve(mm, Y.data(), mm, col.data());
        for (int a = 0; a < mm; a++) W[a + (size_t)mm * j] = col[a];
      }
      std::vector<double> MM((size_t)n * n), qq(n);
      auto QMQ = [&](int i, int j) -> double {                       // Q inv(M) Q' (ICH:1190-1196)
        if (i < nc && j < nc) return G[0][0][(size_t)i * nc + j];
        if (i < nc) return CL[0][(size_t)i * nl + (j - nc)];
        if (j < nc) return CL[0][(size_t)j * nl + (i - nc)];
        return LL[(i - nc) + (size_t)nl * (j - nc)];
      };
      for (int i = 0; i < n; i++) for (int j = 0; j < n; j++) {
        double s = 0.0; for (int a = 0; a < mm; a++) s = s + QX[(size_t)i * mm + a] * W[a + (size_t)mm * j];
        MM[i + (size_t)n * j] = QMQ(i, j) - s;
      }
      std::vector<double> YXv(mm + 1);
      for (int a = 0; a < ns; a++) YXv[a] = Cv[1][Sx[a]];
      for (int a = 0; a < nt; a++) YXv[ns + a] = Cv[2][Tx[a]];
      if (mm > 0) chol_solve(mm, Y.data(), mm, YXv.data());
      for (int i = 0; i < n; i++) {
        double s = 0.0; for (int a = 0; a < mm; a++) s = s + QX[(size_t)i * mm + a] * YXv[a];
        qq[i] = ((i < nc) ? Cv[0][i] : Lv[i - nc]) - s;
      }
      Vec z; z.d.assign(aux->vns, aux->vns + MH_NOSLIP_MAX); z.len = (unsigned)aux->vns_size;
      oracle_rand_t rs; std::memcpy(&rs, aux->rng, sizeof(rs));
      LCP lcp; lcp.rng = &rs;
      Trace tr; tr.buf = trace ? trace + trace_len : nullptr; tr.cap = trace ? ((trace_cap - trace_len > 0) ? trace_cap - trace_len : 0) : 0;
      lcp.trace = &tr;
      unsigned piv = 0;
      bool ok = lcp.lcp_fast(n, MM.data(), n, qq.data(), z, -1.0);
      piv += lcp.pivots;
      if (!ok) { ok = lcp.lcp_lemke_regularized(n, MM.data(), n, qq.data(), z); piv += lcp.pivots; }
      trace_len += tr.len;
      std::memcpy(aux->rng, &rs, sizeof(rs));
      lcp_account(n, piv);
      if (!ok) { aux->status |= MH_WORLD_LCP_FAILED; return false; }
      for (int k = 0; k < n; k++) aux->vns[k] = z[k];
      aux->vns_size = n;
      std::vector<double> t2(mm + 1);                                // [cs; ct] = -(Y^-1 X v + Y^-1 (QX)' z) (ICH:1293-1298)
      for (int a = 0; a < mm; a++) { double s = 0.0; for (int i = 0; i < n; i++) s = s + QX[(size_t)i * mm + a] * z[i]; t2[a] = s; }
      if (mm > 0) chol_solve(mm, Y.data(), mm, t2.data());
      for (int i = 0; i < nc; i++) cn[i] = z[i];
      for (int k = 0; k < nl; k++) l[k] = z[nc + k];
      for (int a = 0; a < ns; a++) csv[Sx[a]] = -(YXv[a] + t2[a]);
      for (int a = 0; a < nt; a++) ctv[Tx[a]] = -(YXv[ns + a] + t2[ns + a]);
      return true;
    };
    // Drumwright-Shell QP -> LCP with contact and limit variables (ICH-QP:94-497) on the persistent _z / _zlast
    auto solve_qp = [&]() -> bool {
      std::vector<double> MM((size_t)N * N, 0.0), qq(N, 0.0);
      auto at = [&](int r, int c2) -> double& { return MM[(size_t)r + (size_t)N * c2]; };
      const int dirs[5] = { 0, 1, 2, 1, 2 }; const double sgn[5] = { 1, 1, 1, -1, -1 };
      for (int a2 = 0; a2 < 5; a2++) {
        for (int b2 = 0; b2 < 5; b2++) for (int i = 0; i < nc; i++) for (int j = 0; j < nc; j++) {
          double g = Gs(dirs[a2], dirs[b2], i, j);
          if (sgn[a2] * sgn[b2] < 0) g = -g;
          at(a2 * nc + i, b2 * nc + j) = g;
        }
        for (int i = 0; i < nc; i++) for (int k = 0; k < nl; k++) {    // Cd X L' and its transpose (ICH-QP:411-434)
          double g = CL[dirs[a2]][(size_t)i * nl + k];
          if (sgn[a2] < 0) g = -g;
          at(a2 * nc + i, 5 * nc + k) = g; at(5 * nc + k, a2 * nc + i) = g;
        }
      }
      for (int a2 = 0; a2 < nl; a2++) for (int b2 = 0; b2 < nl; b2++) at(5 * nc + a2, 5 * nc + b2) = LL[a2 + (size_t)nl * b2];
      for (int i = 0; i < nc; i++) at(i, i) = at(i, i) + m->cp_compliance;                          // ICH-QP:438-440
      for (int i = 0; i < nc; i++) { qq[i] = Cv[0][i]; qq[nc + i] = Cv[1][i]; qq[2*nc + i] = Cv[2][i]; qq[3*nc + i] = -Cv[1][i]; qq[4*nc + i] = -Cv[2][i]; }
      for (int k = 0; k < nl; k++) qq[5 * nc + k] = Lv[k];
      for (int i = 0; i < nc; i++) { for (int c2 = 0; c2 < nvars; c2++) at(nvars + i, c2) = at(i, c2); qq[nvars + i] = Cv[0][i]; }
      for (int k = 0; k < nl; k++) { for (int c2 = 0; c2 < nvars; c2++) at(nvars + nc + k, c2) = at(5 * nc + k, c2); qq[nvars + nc + k] = Lv[k]; }
      int row = nvars + nc + nl;
      for (int i = 0; i < nc; i++) {
        const double vel = std::sqrt(Cv[1][i] * Cv[1][i] + Cv[2][i] * Cv[2][i]);
        for (int j = 0; j < kh; j++) {
          const double theta = (double)j / (kh - 1) * M_PI_2;
          const double ct = std::cos(theta), st_ = std::sin(theta);
          at(row, i) = m->cp_mu_coulomb;
          at(row, nc + i) = -ct; at(row, 3*nc + i) = -ct;
          at(row, 2*nc + i) = -st_; at(row, 4*nc + i) = -st_;
          qq[row] = m->cp_mu_viscous * vel;
          row++;
        }
      }
      for (int r = nvars; r < N; r++) for (int c2 = 0; c2 < nvars; c2++) at(c2, r) = -at(r, c2);
      Vec z; z.d.assign(aux->zbuf, aux->zbuf + aux->zbuf_cap); z.len = (unsigned)aux->zbuf_size;   // solve_qp_work's chain (ICH-QP:157-233)
      z.resize((unsigned)N);
      if ((int)z.size() == aux->zlast_size) for (int i = 0; i < N; i++) z[i] = aux->zlast[i];
      oracle_rand_t rs; std::memcpy(&rs, aux->rng, sizeof(rs));
      LCP lcp; lcp.rng = &rs;
      Trace tr; tr.buf = trace ? trace + trace_len : nullptr; tr.cap = trace ? ((trace_cap - trace_len > 0) ? trace_cap - trace_len : 0) : 0;
      lcp.trace = &tr;
      unsigned piv = 0;
      bool ok = lcp.lcp_fast_regularized(N, MM.data(), N, qq.data(), z, -20, 4, -8);
      piv += lcp.pivots;
      if (!ok) { z.set_zero(); ok = lcp.lcp_lemke_regularized(N, MM.data(), N, qq.data(), z); piv += lcp.pivots; }
      trace_len += tr.len;
      std::memcpy(aux->rng, &rs, sizeof(rs));
      lcp_account(N, piv);
      if (!ok) { aux->status |= MH_WORLD_LCP_FAILED; return false; }   // LCPSolverException
      aux->zlast_size = N;
      for (int i = 0; i < N; i++) { aux->zlast[i] = z[i]; aux->zbuf[i] = z[i]; }
      if (aux->zbuf_cap < N) aux->zbuf_cap = N;
      aux->zbuf_size = nvars;                                          // z repacked to the epd layout = its first N_VARS entries (ICH-QP:236-250)
      return true;
    };
    auto from_stacked = [&]() {                                        // update_from_stacked(q, z) (UCPD:218-228)
      for (int i = 0; i < nc; i++) {
        cn[i] = aux->zbuf[i];
        double sv2 = aux->zbuf[nc + i];   sv2 = sv2 - aux->zbuf[3*nc + i]; csv[i] = sv2;
        double tv2 = aux->zbuf[2*nc + i]; tv2 = tv2 - aux->zbuf[4*nc + i]; ctv[i] = tv2;
      }
      for (int k = 0; k < nl; k++) l[k] = aux->zbuf[5 * nc + k];
    };
    if (noslip) {
      if (!solve_noslip()) return;
      apply(); update_vels();
      const double minv = minv_of();
      bool changed = false;                                            // apply_restitution(q) (ICH:497-525)
      for (int i = 0; i < nc; i++) { cn[i] = cn[i] * m->cp_epsilon; if (!changed && cn[i] > A_NEAR_ZERO) changed = true; }
      for (int k = 0; k < nl; k++) { l[k] = l[k] * m->limit_restitution[idx[k]]; if (!changed && l[k] > A_NEAR_ZERO) changed = true; }
      if (changed) {
        for (int i = 0; i < nc; i++) { csv[i] = 0.0; ctv[i] = 0.0; }
        apply(); update_vels();
        const double minv_plus = minv_of();
        if (minv_plus < 0.0 && minv_plus < minv - A_NEAR_ZERO) aux->status |= MH_WORLD_UNSUPPORTED;
      }
    } else {                                                           // apply_model_to_connected_constraints (ICH:530-626)
      if (!solve_qp()) return;
      from_stacked(); apply(); update_vels();
      const double minv = minv_of();
      bool changed = false;                                            // apply_restitution(q, z) (ICH:470-491): cn and l entries of z only
      for (int i = 0; i < nc; i++) { aux->zbuf[i] = aux->zbuf[i] * m->cp_epsilon; if (!changed && aux->zbuf[i] > A_NEAR_ZERO) changed = true; }
      for (int k = 0; k < nl; k++) { double& zl = aux->zbuf[5 * nc + k]; zl = zl * m->limit_restitution[idx[k]]; if (!changed && zl > A_NEAR_ZERO) changed = true; }
      if (changed) {
        from_stacked(); apply(); update_vels();                        // the tangential impulses are applied again in full, as the reference does
        const double minv_plus = minv_of();
        if (minv_plus < 0.0 && minv_plus < minv - A_NEAR_ZERO) {       // ICH:591-600: second solve on the updated C v vectors
          if (!solve_qp()) return;
          from_stacked(); apply();
        }
      }
    }
    link_velocities(V);                                              // ICH:157-167
    for (int i = 0; i < nc; i++) if (cvel(V, cs[i]) < -A_NEAR_ZERO) aux->status |= MH_WORLD_IMPACT_TOL;
    for (int k = 0; k < nl; k++) { const double v = upper[k] ? -qd[idx[k]] : qd[idx[k]]; if (v < -A_NEAR_ZERO) aux->status |= MH_WORLD_IMPACT_TOL; }
  }
};

// do_mini_step of artic_boxsphere_ref.cpp with every contact's slot beside it and the fold into rep (this world's rows of the step, or NULL)
double do_mini_step_r(ArticR& w, double dt, const mh_artic_drive* D, int B, int b, int s, double* rep)
{
  const mh_artic_model* m = w.m; const int nj = w.nj;
  double qsave[Artic::NJ], V[Artic::NJ][6];
  for (int i = 0; i < nj; i++) qsave[i] = w.q[i];
  double h = 0.0;
  unsigned long guard = 0;
  while (h < dt) {
    if (++guard > MH_CA_HARD_CAP) { w.aux->status |= MH_WORLD_STALLED; break; }
    w.kinematics(); w.link_velocities(V);
    double CA = INF_;
    for (int k = 0; k < m->nspheres; k++) { if (w.masked(k)) continue; const double e = w.CA_sphere(k, V); CA = (e < CA) ? e : CA; }
    for (int k = 0; k < m->nboxes; k++) { if (m->box_link[k] < 0) continue; const double e = CA_box(w, k, V); CA = (e < CA) ? e : CA; }
    for (int k = 0; k < m->npairs; k++) { const double e = w.is_bsp(k) ? w.CA_bsp(k, V) : w.CA_pair(k, V); CA = (e < CA) ? e : CA; }
    if (CA <= 0.0) break;
    double tc = (m->min_step_size > CA) ? m->min_step_size : CA;
    tc = ((dt - h) < tc) ? (dt - h) : tc;
    for (int i = 0; i < nj; i++) { double qn = w.qd[i] * (h + tc); qn = qn + qsave[i]; w.q[i] = qn; }
    h += tc;
  }
  double qdd[Artic::NJ], tau[Artic::NJ];
  const bool driven = drive_tau(D, B, b, s, nj, w.q, w.qd, tau);
  const bool ok = (m->algorithm == MH_ARTIC_FSAB) ? w.fwd_dyn_aba(driven ? tau : nullptr, qdd) : w.fwd_dyn(driven ? tau : nullptr, qdd);
  if (!ok) { w.aux->status |= MH_WORLD_LCP_FAILED; return h; }       // thrown before the contacts exist: nothing to fold
  for (int i = 0; i < nj; i++) w.qd[i] = w.qd[i] + qdd[i] * h;
  std::vector<PC> cs; std::vector<int> slot;           // spheres, then every box's vertices within the threshold, then the pairs
  for (int k = 0; k < m->nspheres; k++) {
    if (w.masked(k)) continue;
    double ctr[3], cp[3]; w.sphere_center(k, ctr); w.to_plane(ctr, cp);
    const double dist = cp[1] + (-1.0 * m->sphere_radius[k]);
    Artic::AContact c;
    if (dist < m->contact_dist_thresh && w.find_contact(k, m->contact_dist_thresh, c)) { cs.push_back(c); slot.push_back(k); }
  }
  for (int k = 0; k < m->nboxes; k++) {
    double pa[3], pp[3];
    if (m->box_link[k] < 0) continue;                  // a static box never meets the plane
    if (!(box_dist(w, k, pa, pp) < m->contact_dist_thresh)) continue;
    for (int i = 0; i < 8; i++) { double v[3], q[3]; box_vertex(w, k, i, v); w.to_plane(v, q); if (q[1] <= m->contact_dist_thresh) { cs.push_back(vertex_contact(w, k, v, q[1])); slot.push_back(m->nspheres + k); } }
  }
  for (int k = 0; k < m->npairs; k++) {
    PC c;
    if (w.is_bsp(k)) { if (w.any_dist(k) < m->contact_dist_thresh && w.bsp_contact(k, m->contact_dist_thresh, c)) { cs.push_back(c); slot.push_back(m->nspheres + m->nboxes + k); } }
    else if (w.pair_contact(k, m->contact_dist_thresh, c) && c.dist < m->contact_dist_thresh) { cs.push_back(c); slot.push_back(m->nspheres + m->nboxes + k); }
  }
  std::vector<double> acc(3 * cs.size() + 1, 0.0);     // a new constraint list: no contact has received an impulse yet
  w.handle_impacts_r(cs, acc);
  if (w.aux->status & MH_WORLD_LCP_FAILED) return h;   // the handler threw: the callback of CSim:353 is not reached
  if (rep) for (size_t c = 0; c < cs.size(); c++) {    // the fold, in constraint-list order
    const bool has = c < (size_t)MH_NOSLIP_MAX;        // the handler holds no more contacts than that: one beyond them has no impulse
    const double cn = has ? acc[3*c] : 0.0, csi = has ? acc[3*c + 1] : 0.0, cti = has ? acc[3*c + 2] : 0.0;
    double* row = rep + (size_t)RP * slot[c];
    row[0] = row[0] + 1.0;
    row[1] = row[1] + cn;
    for (int k = 0; k < 3; k++) { const double jv = (cs[c].n[k] * cn + cs[c].sv[k] * csi) + cs[c].tv[k] * cti; row[2 + k] = row[2 + k] + jv; }
    for (int k = 0; k < 3; k++) row[5 + k] = row[5 + k] + cs[c].p[k] * cn;
  }
  w.aux->time += h; w.aux->mini_steps++; w.folds++;
  return h;
}

void step_r(ArticR& w, double dt, const mh_artic_drive* D, int B, int b, int s, double* rep)
{
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  const int FROZEN = MH_WORLD_UNSUPPORTED | MH_WORLD_STALLED;
  if (w.aux->status & FROZEN) return;
  double h = 0.0; unsigned guard = 0;
  while (h < dt) {
    h += do_mini_step_r(w, dt - h, D, B, b, s, rep);
    if (w.aux->status & MH_WORLD_LCP_FAILED) return;
    if (w.aux->status & FROZEN) break;
    if (++guard > 100000u) { w.aux->status |= MH_WORLD_STALLED; break; }
  }
  stabilize(w);                                        // (adds nothing to the report: it moves positions)
  if (w.aux->status & MH_WORLD_LCP_FAILED) return;
  w.aux->steps++;
}

}  // namespace

extern "C" {

// artic_boxsphere_ref_step with the report: B x nsteps x nslots x MH_REPORT_PAIR doubles (nslots = nspheres + nboxes + npairs), or NULL -- then
// nothing is written and the steps are the same.  Every row of the launch starts at zero; a world that is passed over keeps them zero.
// diag (B x nsteps x 2, or NULL): per world and step the folded mini-steps and the sum of the normal impulses of every handler call's first application.
void artic_report_ref_step(const mh_artic_model* m, int B, double dt, int nsteps, double* q, double* qd, mh_world_aux* aux, double* pose,
                           const mh_artic_drive* drive, double* report, double* diag)
{
  const int nj = m->nj, nslots = m->nspheres + m->nboxes + m->npairs;
  if (report) for (size_t e = 0; e < (size_t)B * nsteps * nslots * RP; e++) report[e] = 0.0;
  for (int b = 0; b < B; b++) {
    double* qb = q + (size_t)b * nj; double* qdb = qd + (size_t)b * nj;
    for (int s = 0; s < nsteps; s++) {
      mh_artic_model mb;
      if (pose) artic_pose_ref_model(m, pose + 7 * (size_t)b, &mb); else std::memcpy(&mb, m, sizeof(mb));
      ArticR w(&mb, qb, qdb, aux + b);
      const unsigned long long done = aux[b].steps;
      step_r(w, dt, drive, B, b, s, report ? report + ((size_t)b * nsteps + s) * nslots * RP : nullptr);
      if (pose && aux[b].steps != done) artic_pose_ref_fold(1, nj, qb, qdb, pose + 7 * (size_t)b);
      if (diag) { diag[((size_t)b * nsteps + s) * 2] = (double)w.folds; diag[((size_t)b * nsteps + s) * 2 + 1] = w.first_cn; }
    }
  }
}

}  // extern "C"
