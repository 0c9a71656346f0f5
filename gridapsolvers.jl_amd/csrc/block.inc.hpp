// block.inc.hpp -- block-diagonal / block-triangular / Schur complement preconditioners and the outer Krylov solve on a
// block system (included at the end of gmg_amd.hip; everything runs on ONE stream of ONE device).
//
// This is SURVEY 8(f)(2): the glue that calls the GMG hot path once per outer FGMRES iteration in
// the reference's Stokes / Navier-Stokes / Darcy applications (test/Applications/StokesGMG.jl:142-153):
//   BlockDiagonalSolver   solve!: src/BlockSolvers/BlockDiagonalSolvers.jl:165-177
//   BlockTriangularSolver solve!: src/BlockSolvers/BlockTriangularSolvers.jl:186-242
//   SchurComplementSolver solve!: src/LinearSolvers/SchurComplementSolvers.jl:55-74 (2 blocks: A = block 0, S = block 1)
// Block vectors are contiguous on the device, block i at off[i]..off[i+1].  Diagonal-block solvers:
// a set-up gmg handle, CGSolver(JacobiLinearSolver()), LUSolver() (small blocks), JacobiLinearSolver(), or a Krylov solver around a
// set-up gmg handle (GMG_BLOCK_KRYLOV_GMG: FGMRESSolver(m,gmg) / GMRESSolver(m;Pr|Pl=gmg) / CGSolver(gmg), NavierStokesGMG.jl:159-169).

struct BlockDiag {
  int kind = 0;                 // gmg_block_diag_kind, 0 = not set
  gmg_solver *g = nullptr;      // GMG_BLOCK_GMG, GMG_BLOCK_KRYLOV_GMG (borrowed)
  int krylov = 0, m = 0, m_add = 1, side = 0;   // GMG_BLOCK_KRYLOV_GMG: gmg_krylov_kind and the solver's sizes (side: 0 = Pr, 1 = Pl)
  bool restart = false, flexible = false;
  int64_t napplies = 0, total_iters = 0;        // gmg_block_diag_stats: since the last gmg_block_setup
  HostCSR hM;                   // matrix of the block solver (MatrixBlock / BiformBlock); empty: system block (i,i)
  bool hasM = false;
  DevCSR M;
  double *dinv = nullptr, *Minv = nullptr;
  int maxiter = 1000;
  double atol = 1e-12, rtol = 1e-6;
  double *w = nullptr, *p = nullptr, *z = nullptr, *r = nullptr;   // CGSolvers.jl:42-48
  ConvLog log;
  bool refresh = false;         // gmg_block_refresh_diag_solver: NonlinearSystemBlock, set up again at the next gmg_block_setup
};

// what gmg_block_update_values[_csc] needs to know about one stored block besides its host copy
struct BlockMeta {
  int layout = GMG_CSR;            // layout the block was set with
  bool dirty = false;              // values changed since the last gmg_block_setup
  std::vector<uint32_t> csc_perm;  // gmg_block_update_values_csc: CSR position of every CSC entry, recorded by the first call
};

struct gmg_block_solver {
  gmg_solver eng;               // stream, allocator, reductions, SpMV launchers (no levels)
  int nb = 0;
  std::vector<int64_t> off;
  int kind = GMG_BLOCK_DIAGONAL;
  std::vector<BlockDiag> diag;
  std::map<std::pair<int, int>, HostCSR> hsys, hpre;
  std::map<std::pair<int, int>, DevCSR> sys, pre;
  std::vector<double> coeff;    // nb*nb row-major, BlockTriangularSolvers.jl:66 (default 1.0)
  double *w = nullptr, *y = nullptr, *tmp = nullptr;               // BlockTriangularSolvers.jl:145-150; Schur: bu, bp in w, du in y
  double *kw = nullptr, *kp = nullptr, *kz = nullptr, *kr = nullptr, *st_b = nullptr, *st_x = nullptr;
  std::vector<double *> fg_V, fg_Z;
  bool setup_done = false;
  std::string err;
  // numerical_setup!(ns,A) (BlockTriangularSolvers.jl:156-186, BlockDiagonalSolvers.jl:153-163): what changed since the last setup
  std::map<std::pair<int, int>, BlockMeta> msys, mpre;
  std::vector<BlockMeta> mdiag;    // of BlockDiag::hM
  bool was_setup = false;          // the device state of the last gmg_block_setup is whole
  bool structure_dirty = true;     // anything but values changed since then
  int info_kind = 0;               // gmg_block_get_setup_info: 1 = full, 2 = in place
  int64_t info_blocks = 0, info_value_bytes = 0;
  // distributed runs (one handle per rank): block vectors hold the OWNED entries of every block; a block whose columns reach
  // into other ranks' entries gets an exchange plan and a work vector with ghost space ([own | ghost], as on GMG levels)
  std::vector<HaloPlan> plan;
  std::vector<double *> xg;

  int64_t N() const { return off.empty() ? 0 : off.back(); }
  int64_t bsize(int i) const { return off[i + 1] - off[i]; }
  int64_t ncols_of(int j) const { return bsize(j) + ((size_t)j < plan.size() && plan[j].present ? plan[j].n_ghost : 0); }
  bool distributed() const { return eng.comm.nranks > 1; }
  // x_j with its ghost entries filled (consistent!): own part copied into the work vector, halo exchanged
  const double *with_ghosts(int j, const double *xj)
  {
    // (a rank without ghosts of its own may still have to SEND: discontinuous pressure spaces -- only "no neighbours" skips the exchange)
    if (!distributed() || (size_t)j >= plan.size() || !plan[j].present || plan[j].nbr.empty()) return xj;
    eng.copy(xg[j], xj, bsize(j));
    eng.exchange_plan(plan[j], xg[j], eng.stream);
    return xg[j];
  }

  void detach()
  {
    for (auto &D : diag)
      if (D.g) {                                           // D.g is nulled by block_forget when its owner destroys it first
        if (D.g->stream == eng.stream) D.g->stream = D.g->own_stream;
        if (D.g->attached_to == this) D.g->attached_to = nullptr;
      }
  }

  void touch() { setup_done = false; structure_dirty = true; }
  BlockMeta &meta_of(int slot, int i, int j) { return slot == GMG_BLOCK_SLOT_SYSTEM ? msys[{i, j}] : slot == GMG_BLOCK_SLOT_PRECOND ? mpre[{i, j}] : mdiag[(size_t)i]; }

  // gmg_block_setup: in place when only values changed and every changed block is stored with explicit values, else in full
  void setup()
  {
    HIP_CHECK(hipSetDevice(eng.device));
    if (can_refresh()) refresh();
    else full_setup();
    for (auto &kv : msys) kv.second.dirty = false;
    for (auto &kv : mpre) kv.second.dirty = false;
    for (auto &m : mdiag) m.dirty = false;
    for (auto &D : diag) { D.refresh = false; D.napplies = 0; D.total_iters = 0; }
  }

  // the device form of a dirty block (nullptr: it has none, e.g. the matrix of an LU block)
  DevCSR *dirty_dev(int slot, int i, int j)
  {
    if (slot == GMG_BLOCK_SLOT_DIAG_MATRIX) return (diag[i].kind == GMG_BLOCK_CG_JACOBI || diag[i].kind == GMG_BLOCK_JACOBI) ? &diag[i].M : nullptr;
    auto &m = slot == GMG_BLOCK_SLOT_SYSTEM ? sys : pre;
    auto it = m.find({i, j});
    return it == m.end() ? nullptr : &it->second;
  }
  template <typename F>
  void for_each_dirty(F &&f)                                 // f(slot, i, j, host copy)
  {
    for (auto &kv : msys) if (kv.second.dirty) f((int)GMG_BLOCK_SLOT_SYSTEM, kv.first.first, kv.first.second, hsys.at(kv.first));
    for (auto &kv : mpre) if (kv.second.dirty) f((int)GMG_BLOCK_SLOT_PRECOND, kv.first.first, kv.first.second, hpre.at(kv.first));
    for (int i = 0; i < nb; ++i) if (mdiag[(size_t)i].dirty && diag[i].hasM) f((int)GMG_BLOCK_SLOT_DIAG_MATRIX, i, i, diag[i].hM);
  }
  // the matrix a Jacobi / CG-Jacobi / LU block is set up on: its own (MatrixBlock) or the system's (i,i)
  int diag_slot(int i) const { return diag[i].hasM ? GMG_BLOCK_SLOT_DIAG_MATRIX : GMG_BLOCK_SLOT_SYSTEM; }

  bool can_refresh()
  {
    if (!was_setup || structure_dirty || eng.comm.nranks != 1 || !eng.opt_int("GMG_REFRESH", 1)) return false;
    // a marked Jacobi block takes D^-1 from the refill of its matrix: that matrix is written again whether or not it changed
    for (int i = 0; i < nb; ++i)
      if (diag[i].refresh && (diag[i].kind == GMG_BLOCK_CG_JACOBI || diag[i].kind == GMG_BLOCK_JACOBI)) meta_of(diag_slot(i), i, i).dirty = true;
    bool ok = true;
    for_each_dirty([&](int slot, int i, int j, const HostCSR &) {
      const DevCSR *M = dirty_dev(slot, i, j);
      if (M && !M->explicit_values()) ok = false;            // dictionary / row-pattern layout: chosen from the values
    });
    return ok;
  }

  // numerical_setup!(ns,A) in place: every layout, work vector, Krylov basis, exchange plan and attachment stays; the values of the
  // dirty blocks are copied to the device and refilled, the MARKED diagonal solvers (NonlinearSystemBlock) are set up again, the
  // others keep their D^-1 / inverse (LinearSystemBlock / MatrixBlock: BlockSolverInterfaces.jl:104-118,232-236)
  void refresh()
  {
    const bool timing = eng.opt_int("GMG_SETUP_TIMING", 0) != 0;
    const auto t_begin = std::chrono::steady_clock::now();
    gmg_solver::RefillStage st;
    st.timed = timing;
    double solver_ms = 0.0;
    info_kind = 2; info_blocks = 0; info_value_bytes = 0;
    setup_done = false;
    try {
      for_each_dirty([&](int slot, int i, int j, const HostCSR &H) {
        DevCSR *M = dirty_dev(slot, i, j);
        if (!M) return;
        double *dinv = nullptr;
        if (i == j && diag[i].refresh && slot == diag_slot(i) && diag[i].dinv) dinv = diag[i].dinv;
        int nzero = 0;
        if (st.d_nzero) HIP_CHECK(hipMemsetAsync(st.d_nzero, 0, sizeof(int), eng.stream));
        eng.refill_values(*M, H.val.data(), dinv, st);
        if (dinv) {
          HIP_CHECK(hipMemcpyAsync(&nzero, st.d_nzero, sizeof(int), hipMemcpyDeviceToHost, eng.stream));
          HIP_CHECK(hipStreamSynchronize(eng.stream));
          REQUIRE(nzero == 0, GMG_ERR_SINGULAR, "zero diagonal entry in block " + std::to_string(i));
        }
        info_blocks += 1; info_value_bytes += (int64_t)sizeof(double) * H.nnz();
      });
      const auto t_solvers = std::chrono::steady_clock::now();
      for (int i = 0; i < nb; ++i) {
        BlockDiag &D = diag[i];
        if (!D.refresh) continue;
        if (D.kind == GMG_BLOCK_GMG || D.kind == GMG_BLOCK_KRYLOV_GMG)   // the caller has refreshed the GMG handle itself (gmg_update_values* + gmg_setup)
          REQUIRE(D.g && D.g->setup_done, GMG_ERR_STATE, "the GMG handle of block " + std::to_string(i) + " is not set up");
        else if (D.kind == GMG_BLOCK_LU) {
          HIP_CHECK(hipStreamSynchronize(eng.stream));
          eng.release(D.Minv, (size_t)bsize(i) * (size_t)bsize(i));
          D.Minv = eng.build_dense_inverse(D.hasM ? D.hM : hsys.at({i, i}), "diagonal block " + std::to_string(i));
        }
      }
      HIP_CHECK(hipStreamSynchronize(eng.stream));
      solver_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_solvers).count();
    } catch (...) {
      eng.refill_release(st);
      structure_dirty = true;                                // half-written: the next gmg_block_setup is a full one
      throw;
    }
    eng.refill_release(st);
    setup_done = true;
    if (timing)
      std::fprintf(stderr, "[gmg_block_setup] in place: %lld blocks, copy %8.1f ms, refill (+ D^-1) %8.1f ms, inverses %8.1f ms, total %8.1f ms\n",
                   (long long)info_blocks, st.copy_ms, st.fill_ms, solver_ms,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  }

  void full_setup()
  {
    const bool timing = eng.opt_int("GMG_SETUP_TIMING", 0) != 0;
    const auto t_begin = std::chrono::steady_clock::now();
    if (kind == GMG_BLOCK_SCHUR) {
      REQUIRE(!distributed(), GMG_ERR_UNSUPPORTED, "the Schur complement solver is single-GPU (no partitioned application)");
      // SchurComplementSolvers.jl:16-19: B and C are arguments of the solver; here the precond block or, without one, the system's
      REQUIRE(hpre.count({0, 1}) || hsys.count({0, 1}), GMG_ERR_STATE, "Schur complement solver: block (0,1) (B) is missing: no precond block and no system block");
      REQUIRE(hpre.count({1, 0}) || hsys.count({1, 0}), GMG_ERR_STATE, "Schur complement solver: block (1,0) (C) is missing: no precond block and no system block");
    }
    // a Krylov solver around a GMG: the nested solve uses the GMG handle's scalar slots, mailbox and basis caches and reduces on its own rank only
    for (int i = 0; i < nb; ++i)
      if (diag[i].kind == GMG_BLOCK_KRYLOV_GMG)
        REQUIRE(!distributed() && (!diag[i].g || diag[i].g->comm.nranks == 1), GMG_ERR_UNSUPPORTED,
                "the Krylov solver around the GMG of block " + std::to_string(i) + " is single-GPU (no partitioned nested solve)");
    // State that numerical_setup! keeps (the reference's work caches): y -- the initial guesses of the CG block solvers and the
    // Schur solver's du -- on every later setup; and, when only values changed (the fallback of the in-place path), D^-1 / the
    // inverse of the diagonal solvers that are NOT marked, so that both paths of gmg_block_setup give the same bits.
    const bool values_only = was_setup && !structure_dirty;
    std::vector<double> keep_y;
    std::vector<std::vector<double>> keep_solver((size_t)nb);
    if (y) {
      HIP_CHECK(hipStreamSynchronize(eng.stream));
      keep_y.resize((size_t)N());
      if (N() > 0) HIP_CHECK(hipMemcpy(keep_y.data(), y, sizeof(double) * (size_t)N(), hipMemcpyDeviceToHost));
      if (values_only)
        for (int i = 0; i < nb; ++i) {
          const BlockDiag &D = diag[i];
          const double *src = D.kind == GMG_BLOCK_LU ? D.Minv : (D.kind == GMG_BLOCK_CG_JACOBI || D.kind == GMG_BLOCK_JACOBI) ? D.dinv : nullptr;
          if (D.refresh || !src) continue;
          keep_solver[(size_t)i].resize(D.kind == GMG_BLOCK_LU ? (size_t)bsize(i) * (size_t)bsize(i) : (size_t)bsize(i));
          if (!keep_solver[(size_t)i].empty())
            HIP_CHECK(hipMemcpy(keep_solver[(size_t)i].data(), src, sizeof(double) * keep_solver[(size_t)i].size(), hipMemcpyDeviceToHost));
        }
    }
    was_setup = false;
    detach();
    eng.free_all();
    w = y = tmp = nullptr;
    for (auto &D : diag) { D.dinv = D.Minv = nullptr; D.M = DevCSR(); }
    sys.clear(); pre.clear();
    info_kind = 1; info_blocks = 0; info_value_bytes = 0;
    for (auto &kv : hsys) { info_blocks += 1; info_value_bytes += (int64_t)sizeof(double) * kv.second.nnz(); }
    for (auto &kv : hpre) { info_blocks += 1; info_value_bytes += (int64_t)sizeof(double) * kv.second.nnz(); }
    eng.read_tuning();
    eng.init_reductions();
    int64_t nmax = 1;
    for (int i = 0; i < nb; ++i) nmax = std::max(nmax, bsize(i));
    xg.assign((size_t)nb, nullptr);
    if (distributed()) {
      plan.resize((size_t)nb);
      for (int j = 0; j < nb; ++j)
        if (plan[j].present) {
          REQUIRE(plan[j].n_own == bsize(j), GMG_ERR_INVALID, "partition of block " + std::to_string(j) + " does not match its size");
          plan[j].d_snd_idx = nullptr; plan[j].d_sendbuf = nullptr; plan[j].d_recvbuf = nullptr;
          eng.alloc_plan_buffers(plan[j]);
          xg[j] = eng.dvec(bsize(j) + plan[j].n_ghost);
        }
    }
    for (auto &kv : hsys) sys[kv.first] = eng.upload_csr(kv.second);
    for (auto &kv : hpre) pre[kv.first] = eng.upload_csr(kv.second);
    for (int i = 0; i < nb; ++i) {
      BlockDiag &D = diag[i];
      REQUIRE(D.kind != 0, GMG_ERR_STATE, "no solver set for diagonal block " + std::to_string(i));
      const int64_t n = bsize(i);
      if (D.kind == GMG_BLOCK_GMG || D.kind == GMG_BLOCK_KRYLOV_GMG) {
        gmg_solver *g = D.g;
        if (D.kind == GMG_BLOCK_KRYLOV_GMG)
          REQUIRE(!g || !g->has_outer(), GMG_ERR_UNSUPPORTED, "the GMG handle of block " + std::to_string(i) + " has its finest level in the overlapping layout");
        REQUIRE(g && g->setup_done, GMG_ERR_STATE, "the GMG handle of block " + std::to_string(i) + " is not set up");
        REQUIRE(g->device == eng.device, GMG_ERR_INVALID, "GMG handle lives on another device");
        REQUIRE(g->comm.nranks == eng.comm.nranks, GMG_ERR_INVALID, "the GMG handle of block " + std::to_string(i) + " and the block solver must span the same ranks");
        REQUIRE(g->lev[0].n == n, GMG_ERR_INVALID, "GMG handle size does not match block " + std::to_string(i));
        HIP_CHECK(hipStreamSynchronize(g->stream));
        REQUIRE(g->attached_to == nullptr || g->attached_to == this, GMG_ERR_STATE, "GMG handle is already attached to another block solver");
        g->stream = eng.stream;                           // one stream: block glue and V-cycles are ordered without events
        g->attached_to = this;
        continue;
      }
      const HostCSR *src = nullptr;
      if (D.hasM) src = &D.hM;
      else {
        auto it = hsys.find({i, i});
        REQUIRE(it != hsys.end(), GMG_ERR_STATE, "block " + std::to_string(i) + ": no solver matrix and no system block (i,i)");
        src = &it->second;
      }
      REQUIRE(src->nrows == n && src->ncols == ncols_of(i), GMG_ERR_INVALID, "solver matrix of block " + std::to_string(i) + " has the wrong shape");
      if (D.kind == GMG_BLOCK_LU) {
        REQUIRE(!distributed(), GMG_ERR_UNSUPPORTED, "LUSolver() diagonal blocks are single-GPU (a dense inverse of a distributed block is not formed)");
        D.Minv = eng.build_dense_inverse(*src, "diagonal block " + std::to_string(i));
        continue;
      }
      // LinearSystemBlock: the solver streams the system's own (i,i) block, uploaded once
      DevCSR &M = D.hasM ? (D.M = eng.upload_csr(*src)) : sys[{i, i}];
      int nzero = 0;
      D.dinv = eng.build_inv_diag(M, nzero);
      REQUIRE(nzero == 0 || !keep_solver[(size_t)i].empty(), GMG_ERR_SINGULAR, "zero diagonal entry in block " + std::to_string(i));
      if (D.hasM) { eng.drop_csr_stream(D.M); info_blocks += 1; info_value_bytes += (int64_t)sizeof(double) * src->nnz(); }
      if (D.kind == GMG_BLOCK_CG_JACOBI) { D.w = eng.dvec(n); D.p = eng.dvec(n); D.z = eng.dvec(n); D.r = eng.dvec(n); }
    }
    for (auto &kv : sys) eng.drop_csr_stream(kv.second);
    for (auto &kv : pre) eng.drop_csr_stream(kv.second);
    for (int i = 0; i < nb; ++i)
      if (!diag[i].hasM && (diag[i].kind == GMG_BLOCK_CG_JACOBI || diag[i].kind == GMG_BLOCK_JACOBI)) diag[i].M = sys[{i, i}];
    const int64_t n = N();
    w = eng.dvec(n); y = eng.dvec(n); tmp = eng.dvec(nmax);
    kw = eng.dvec(n); kp = eng.dvec(n); kz = eng.dvec(n); kr = eng.dvec(n);
    st_b = eng.dvec(n); st_x = eng.dvec(n);
    fg_V.clear(); fg_Z.clear();
    if (!keep_y.empty()) HIP_CHECK(hipMemcpyAsync(y, keep_y.data(), sizeof(double) * keep_y.size(), hipMemcpyHostToDevice, eng.stream));
    for (int i = 0; i < nb; ++i)
      if (!keep_solver[(size_t)i].empty())
        HIP_CHECK(hipMemcpyAsync(diag[i].kind == GMG_BLOCK_LU ? diag[i].Minv : diag[i].dinv, keep_solver[(size_t)i].data(),
                                 sizeof(double) * keep_solver[(size_t)i].size(), hipMemcpyHostToDevice, eng.stream));
    HIP_CHECK(hipStreamSynchronize(eng.stream));
    setup_done = true;
    was_setup = true;
    structure_dirty = false;
    if (timing)
      std::fprintf(stderr, "[gmg_block_setup] full: %lld blocks, total %8.1f ms\n", (long long)info_blocks,
                   std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_begin).count());
  }

  const DevCSR *sys_block(int i, int j) const
  {
    auto it = sys.find({i, j});
    return it == sys.end() ? nullptr : &it->second;
  }
  // off-diagonal block of the PRECONDITIONER: an explicit one (MatrixBlock / BiformBlock) or the
  // system's (LinearSystemBlock, BlockSolverInterfaces.jl)
  const DevCSR *pre_block(int i, int j) const
  {
    auto it = pre.find({i, j});
    if (it != pre.end()) return &it->second;
    return sys_block(i, j);
  }

  // y = A x, block-wise
  void sys_apply(const double *x, double *yv)
  {
    for (int i = 0; i < nb; ++i) {
      bool first = true;
      double *yi = yv + off[i];
      for (int j = 0; j < nb; ++j) {
        const DevCSR *M = sys_block(i, j);
        if (!M) continue;
        const double *xj = with_ghosts(j, x + off[j]);
        if (first) eng.spmv_set(*M, xj, yi);
        else eng.spmv_addto(*M, xj, tmp, yi);
        first = false;
      }
      if (first) eng.zero(yi, bsize(i));
    }
  }
  // r = b - A x
  void sys_resid(const double *x, const double *b, double *r)
  {
    for (int i = 0; i < nb; ++i) {
      bool first = true;
      double *ri = r + off[i];
      for (int j = 0; j < nb; ++j) {
        const DevCSR *M = sys_block(i, j);
        if (!M) continue;
        const double *xj = with_ghosts(j, x + off[j]);
        if (first) eng.spmv_resid(*M, xj, b + off[i], ri);
        else eng.spmv_sub(*M, xj, ri);
        first = false;
      }
      if (first) eng.copy(ri, b + off[i], bsize(i));
    }
  }

  // solve!(yi,nsi,wi) for one diagonal block
  void diag_solve(int i, double *yi, const double *wi)
  {
    BlockDiag &D = diag[i];
    const int64_t n = bsize(i);
    switch (D.kind) {
    case GMG_BLOCK_GMG:
      if (D.g->comm.nranks > 1) {                           // distributed handle: its solution vector carries ghost space
        if (D.g->mode == GMG_MODE_SOLVER) eng.copy(D.g->cg_x, yi, n);
        D.g->gmg_solve_dev(D.g->cg_x, wi, -1.0);
        eng.copy(yi, D.g->cg_x, n);
      } else
      D.g->gmg_solve_dev(yi, wi, -1.0);
      D.napplies += 1; D.total_iters += D.g->log.num_iters;
      break;
    case GMG_BLOCK_KRYLOV_GMG: {
      // solve!(yi,ns,wi) of FGMRESSolver(m,gmg) / GMRESSolver(m;Pr|Pl=gmg) / CGSolver(gmg) on the GMG handle's own finest matrix: the
      // operator, caches (fg_V / fg_Z, gm_*, cg_*), scalar slots and mailbox of gmg_fgmres_solve / gmg_gmres_solve / gmg_cg_solve, on
      // the block handle's stream.  The outer solve reduces on the block engine: the two never share a slot.  Slots on the GMG handle:
      // FGMRES / GMRES 1..j+1, norm / dot 0, a nested cg_core kScalarSlots - 8*depth (the GMG's coarsest CG-Jacobi one depth further).
      // yi keeps its previous content: the initial guess (FGMRESSolvers.jl:136, GMRESSolvers.jl:143, CGSolvers.jl:79).
      gmg_solver &S = *D.g;
      D.log.configure(D.maxiter, D.atol, D.rtol);
      if (D.krylov == GMG_KRYLOV_CG) {
        KrylovOps ops = S.level0_ops(1);
        cg_core(S, n, wi, yi, S.cg_w, S.cg_p, S.cg_z, S.cg_r, ops, D.flexible, D.log);
      } else if (D.krylov == GMG_KRYLOV_FGMRES) {
        KrylovOps ops = S.level0_ops(1);
        fgmres_core(S, n, S.lev[0].nvec, wi, yi, S.fg_V, S.fg_Z, ops, D.m, D.restart, D.m_add, D.log, true);
      } else {
        KrylovOps ops = S.level0_ops(D.side == 0 ? 1 : 0);
        if (D.side == 1) ops.precond_left = [&S](double *z, const double *r) { S.krylov_precond(1, z, r, -1.0); };
        gmres_core(S, n, S.lev[0].nvec, wi, yi, ops, D.m, D.restart, D.m_add, D.log);
      }
      D.napplies += 1; D.total_iters += D.log.num_iters;
      break;
    }
    case GMG_BLOCK_CG_JACOBI: {                           // yi keeps its previous content: CG's initial guess
      KrylovOps ops;
      ops.resid = [&, i](double *x, const double *b, double *r) { eng.spmv_resid(D.M, with_ghosts(i, x), b, r); };
      ops.apply = [&, i](double *x, double *yv) { eng.spmv_set(D.M, with_ghosts(i, x), yv); };
      ops.precond = [&, n](double *z, const double *r, double) {
        hipLaunchKernelGGL(jacobi_apply_kernel, dim3(gmg_solver::grid_for(n)), dim3(256), 0, eng.stream, n, D.dinv, r, z);
        HIP_CHECK(hipGetLastError());
      };
      D.log.configure(D.maxiter, D.atol, D.rtol);
      cg_core(eng, n, wi, yi, D.w, D.p, D.z, D.r, ops, false, D.log);
      D.napplies += 1; D.total_iters += D.log.num_iters;
      break;
    }
    case GMG_BLOCK_LU:
      eng.dense_solve(D.Minv, (int)n, wi, yi);
      break;
    case GMG_BLOCK_JACOBI:
      hipLaunchKernelGGL(jacobi_apply_kernel, dim3(gmg_solver::grid_for(n)), dim3(256), 0, eng.stream, n, D.dinv, wi, yi);
      HIP_CHECK(hipGetLastError());
      break;
    default:
      throw GmgError{GMG_ERR_STATE, "diagonal block solver not set"};
    }
  }

  // solve!(x,ns,y): SchurComplementSolvers.jl:55-74.  The solves of :65 and :67 write into the caller's x, whose content on entry is
  // the initial guess of an iterative block solver; du (the y range of block 0) persists between applications (ns.caches, :58)
  void schur_apply(double *x, const double *b)
  {
    const DevCSR *Bm = pre_block(0, 1), *Cm = pre_block(1, 0);
    const int64_t nu = bsize(0);
    double *xu = x + off[0], *xp = x + off[1];
    double *du = y + off[0], *bu = w + off[0], *bp = w + off[1];             // :58 du,bu,bp = ns.caches
    diag_solve(0, xu, b + off[0]);                                           // :65 solve!(x_u,A,y_u)
    eng.spmv_resid(*Cm, xu, b + off[1], bp);                                 // :66 copy!(bp,y_p); mul!(bp,C,x_u,-1.0,1.0)
    diag_solve(1, xp, bp);                                                   // :67 solve!(x_p,S,bp)
    eng.spmv_set(*Bm, xp, bu);                                               // :69 mul!(bu,B,x_p)
    diag_solve(0, du, bu);                                                   // :70 solve!(du,A,bu)
    hipLaunchKernelGGL(axpy_kernel, dim3(gmg_solver::grid_for(nu)), dim3(256), 0, eng.stream, nu, -1.0, du, xu);   // :71 x_u .-= du
    HIP_CHECK(hipGetLastError());
  }

  // solve!(x,ns,b): BlockDiagonalSolvers.jl:165-177 / BlockTriangularSolvers.jl:186-242
  void precond_apply(double *x, const double *b)
  {
    if (kind == GMG_BLOCK_SCHUR) { schur_apply(x, b); return; }
    for (int step = 0; step < nb; ++step) {
      const int iB = (kind == GMG_BLOCK_UPPER) ? nb - 1 - step : step;       // :218 NB:-1:1 / :190 1:NB
      const int64_t n = bsize(iB);
      const double *rhs = b + off[iB];
      double *yi = y + off[iB];
      if (kind != GMG_BLOCK_DIAGONAL) {
        double *wi = w + off[iB];
        bool touched = false;
        const int j0 = (kind == GMG_BLOCK_UPPER) ? iB + 1 : 0, j1 = (kind == GMG_BLOCK_UPPER) ? nb : iB;
        for (int jB = j0; jB < j1; ++jB) {
          const double cij = coeff[(size_t)iB * nb + jB];
          const double eps = std::nextafter(std::fabs(cij), INFINITY) - std::fabs(cij);   // eps(cij)
          const DevCSR *M = pre_block(iB, jB);
          if (!(std::fabs(cij) > eps) || !M) continue;                       // :194,223
          if (!touched) { eng.copy(wi, rhs, n); touched = true; }            // :192,221 copy!(wi,bi)
          const double *xj = with_ghosts(jB, x + off[jB]);
          if (cij == 1.0) eng.spmv_sub(*M, xj, wi);                          // :196,225 mul!(wi,M,xj,-cij,1.0)
          else {
            eng.spmv_set(*M, xj, tmp);
            hipLaunchKernelGGL(axpy_kernel, dim3(gmg_solver::grid_for(n)), dim3(256), 0, eng.stream, n, -cij, tmp, wi);
            HIP_CHECK(hipGetLastError());
          }
        }
        if (touched) rhs = wi;                                               // no contribution: wi == bi, skip the copy
      }
      diag_solve(iB, yi, rhs);                                               // :202-205,231-234 solve!(yi,nsi,wi)
      eng.copy(x + off[iB], yi, n);                                          // copy!(xi,yi)
    }
  }

  KrylovOps ops(bool use_precond)
  {
    KrylovOps o;
    o.resid = [this](double *x, const double *b, double *r) { sys_resid(x, b, r); };
    o.apply = [this](double *x, double *yv) { sys_apply(x, yv); };
    if (use_precond) o.precond = [this](double *z, const double *r, double) { precond_apply(z, r); };
    return o;
  }
  // gmg_solver::krylov_entry for the block system (vectors of length N(), one rank): the handle's own staging vectors, no retry
  template <typename F>
  void krylov_entry(const double *b, double *x, int memspace, int maxiter, double atol, double rtol, gmg_result *res, double *hist,
                    int hist_cap, F &&body)
  {
    const int64_t n = N();
    const double *db = eng.in_vec(b, n, memspace, st_b);
    double *dx = (memspace == GMG_MEM_DEVICE) ? x : st_x;
    if (memspace == GMG_MEM_HOST) eng.h2d(dx, x, n);       // x = initial guess on entry
    if (eng.ns.project_guess) eng.ns_project_guess(dx, n, false);   // NullspaceSolvers.jl:115-116
    ConvLog log;
    log.configure(maxiter, atol, rtol);
    const double last = body(n, db, dx, log);
    eng.out_vec(x, dx, n, memspace);
    log.export_to(res, hist, hist_cap, last);
  }
};

// gmg_destroy on a handle that a block solver still borrows: drop the pointer, the block solver must be set up again
static void block_forget(gmg_block_solver *B, gmg_solver *g)
{
  for (auto &D : B->diag)
    if (D.g == g) { D.g = nullptr; D.kind = 0; B->touch(); }
  g->attached_to = nullptr;
  if (g->stream == B->eng.stream) {
    (void)hipStreamSynchronize(B->eng.stream);
    g->stream = g->own_stream;
  }
}

namespace {
template <typename F>
int guarded_b(gmg_block_handle_t h, F &&f)
{
  try {
    if (h) HIP_CHECK(hipSetDevice(h->eng.device));
    f();
    return GMG_OK;
  } catch (const GmgError &e) {
    if (h) h->err = e.msg;
    g_last_error = e.msg;
    return e.code;
  } catch (const std::bad_alloc &) {
    if (h) h->err = "host allocation failed";
    g_last_error = "host allocation failed";
    return GMG_ERR_ALLOC;
  } catch (const std::exception &e) {
    if (h) h->err = e.what();
    g_last_error = e.what();
    return GMG_ERR_INVALID;
  }
}
void check_block(gmg_block_handle_t h, int i)
{
  REQUIRE(h, GMG_ERR_INVALID, "null handle");
  REQUIRE(i >= 0 && i < h->nb, GMG_ERR_INVALID, "block index out of range");
}
void check_block_ready(gmg_block_handle_t h)
{
  REQUIRE(h, GMG_ERR_INVALID, "null handle");
  REQUIRE(h->setup_done, GMG_ERR_STATE, "gmg_block_setup has not been called (numerical_setup missing)");
}
} // namespace

extern "C" {

int gmg_block_create(gmg_block_handle_t *out, int nblocks, const int64_t *block_sizes, int kind, int device_id)
{
  return guarded_b(nullptr, [&] {
    REQUIRE(out, GMG_ERR_INVALID, "null handle pointer");
    *out = nullptr;
    REQUIRE(nblocks >= 1 && block_sizes, GMG_ERR_INVALID, "at least one block required");
    REQUIRE(kind == GMG_BLOCK_DIAGONAL || kind == GMG_BLOCK_LOWER || kind == GMG_BLOCK_UPPER || kind == GMG_BLOCK_SCHUR, GMG_ERR_INVALID,
            "kind must be diagonal, :lower or :upper (BlockTriangularSolvers.jl:63) or Schur complement");
    REQUIRE(kind != GMG_BLOCK_SCHUR || nblocks == 2, GMG_ERR_INVALID, "the Schur complement solver takes 2 blocks (SchurComplementSolvers.jl:60)");
    int ndev = 0;
    HIP_CHECK(hipGetDeviceCount(&ndev));
    REQUIRE(ndev > 0, GMG_ERR_HIP, "no HIP device visible: libgmgamd has no CPU path");
    REQUIRE(device_id >= 0 && device_id < ndev, GMG_ERR_INVALID, "device_id out of range");
    HIP_CHECK(hipSetDevice(device_id));
    gmg_block_solver *s = new gmg_block_solver();
    s->eng.device = device_id;
    s->nb = nblocks;
    s->kind = kind;
    s->off.assign((size_t)nblocks + 1, 0);
    for (int i = 0; i < nblocks; ++i) {
      if (block_sizes[i] < 0) { delete s; throw GmgError{GMG_ERR_INVALID, "negative block size"}; }
      s->off[i + 1] = s->off[i] + block_sizes[i];
    }
    s->diag.resize(nblocks);
    s->mdiag.resize(nblocks);
    s->coeff.assign((size_t)nblocks * nblocks, 1.0);
    hipError_t e = hipStreamCreateWithFlags(&s->eng.stream, hipStreamNonBlocking);
    if (e != hipSuccess) {
      delete s;
      throw GmgError{GMG_ERR_HIP, std::string("hipStreamCreate: ") + hipGetErrorString(e)};
    }
    s->eng.own_stream = s->eng.stream;
    *out = s;
  });
}

int gmg_block_destroy(gmg_block_handle_t h)
{
  // borrowed GMG handles destroyed earlier have already been forgotten (block_forget): no dangling pointer is touched
  if (!h) return GMG_OK;
  (void)hipSetDevice(h->eng.device);
  (void)hipStreamSynchronize(h->eng.stream);
  h->detach();                                            // GMG handles get their own stream back
  h->eng.ns_clear();
  h->eng.free_all();
  for (auto &P : h->plan) {
    if (P.h_send) (void)hipHostFree(P.h_send);
    if (P.h_recv) (void)hipHostFree(P.h_recv);
  }
  if (h->eng.comm.kind == COMM_RCCL && h->eng.comm.comm) (void)h->eng.comm.api.CommDestroy(h->eng.comm.comm);
  if (h->eng.comm_stream) (void)hipStreamSynchronize(h->eng.comm_stream);   // created by gmg_block_comm_init_* on the engine
  if (h->eng.ev_ready) (void)hipEventDestroy(h->eng.ev_ready);
  if (h->eng.ev_done) (void)hipEventDestroy(h->eng.ev_done);
  if (h->eng.comm_stream) (void)hipStreamDestroy(h->eng.comm_stream);
  if (h->eng.h_rep_full) (void)hipHostFree(h->eng.h_rep_full);
  if (h->eng.h_scalars) (void)hipHostFree(h->eng.h_scalars);
  if (h->eng.h_mail_col) (void)hipHostFree(h->eng.h_mail_col);
  if (h->eng.own_stream) (void)hipStreamDestroy(h->eng.own_stream);
  delete h;
  return GMG_OK;
}

const char *gmg_block_last_error(gmg_block_handle_t h) { return h ? h->err.c_str() : g_last_error.c_str(); }

// ---- distributed block systems: one handle per rank ------------------------------------------------------------------
int gmg_block_comm_init_rccl(gmg_block_handle_t h, const char *rccl_path, const char *unique_id128, int rank, int nranks)
{
  if (!h) return GMG_ERR_INVALID;
  const int st = gmg_comm_init_rccl(&h->eng, rccl_path, unique_id128, rank, nranks);
  if (st != GMG_OK) h->err = h->eng.err;
  h->touch();
  return st;
}
int gmg_block_comm_init_host(gmg_block_handle_t h, int rank, int nranks, gmg_host_exchange_fn xfn, gmg_host_allreduce_fn rfn, void *ctx)
{
  if (!h) return GMG_ERR_INVALID;
  const int st = gmg_comm_init_host(&h->eng, rank, nranks, xfn, rfn, ctx);
  if (st != GMG_OK) h->err = h->eng.err;
  h->touch();
  return st;
}
int gmg_block_comm_set_loopback(gmg_block_handle_t h, int virtual_nranks)
{
  if (!h) return GMG_ERR_INVALID;
  const int st = gmg_comm_set_loopback(&h->eng, virtual_nranks);
  if (st != GMG_OK) h->err = h->eng.err;
  h->touch();
  return st;
}
int gmg_block_set_partition(gmg_block_handle_t h, int j, int64_t n_own, int64_t n_ghost, int nnbr, const int32_t *nbr_rank,
                            const int64_t *snd_ptr, const int64_t *snd_idx, const int64_t *rcv_ptr)
{
  return guarded_b(h, [&] {
    check_block(h, j);
    REQUIRE(h->eng.comm.nranks > 1, GMG_ERR_STATE, "gmg_block_comm_init_* first");
    REQUIRE(n_own == h->bsize(j), GMG_ERR_INVALID, "n_own must equal the block size given to gmg_block_create");
    if (h->plan.size() < (size_t)h->nb) h->plan.resize((size_t)h->nb);
    fill_plan(h->plan[j], h->eng.comm, n_own, n_ghost, nnbr, nbr_rank, snd_ptr, snd_idx, rcv_ptr);
    h->touch();
  });
}

int gmg_block_set_system_block(gmg_block_handle_t h, int i, int j, int64_t nrows, int64_t ncols, int64_t nnz, const void *ptr,
                               const void *idx, const double *val, int layout, int index_base, int index_bytes)
{
  return guarded_b(h, [&] {
    check_block(h, i); check_block(h, j);
    REQUIRE(nrows == h->bsize(i) && ncols == h->ncols_of(j), GMG_ERR_INVALID, "block shape does not match the block sizes (columns = own + ghost entries of block j)");
    h->hsys[{i, j}] = convert_input(nrows, ncols, nnz, ptr, idx, val, layout, index_base, index_bytes);
    h->msys[{i, j}] = BlockMeta();
    h->msys[{i, j}].layout = layout;
    h->touch();
  });
}

int gmg_block_set_precond_block(gmg_block_handle_t h, int i, int j, int64_t nrows, int64_t ncols, int64_t nnz, const void *ptr,
                                const void *idx, const double *val, int layout, int index_base, int index_bytes)
{
  return guarded_b(h, [&] {
    check_block(h, i); check_block(h, j);
    REQUIRE(i != j, GMG_ERR_INVALID, "diagonal blocks are given with gmg_block_set_diag_*");
    REQUIRE(nrows == h->bsize(i) && ncols == h->ncols_of(j), GMG_ERR_INVALID, "block shape does not match the block sizes (columns = own + ghost entries of block j)");
    h->hpre[{i, j}] = convert_input(nrows, ncols, nnz, ptr, idx, val, layout, index_base, index_bytes);
    h->mpre[{i, j}] = BlockMeta();
    h->mpre[{i, j}].layout = layout;
    h->touch();
  });
}

int gmg_block_set_coeff(gmg_block_handle_t h, int i, int j, double c)
{
  return guarded_b(h, [&] {
    check_block(h, i); check_block(h, j);
    double &cij = h->coeff[(size_t)i * h->nb + j];
    if ((cij == 0.0) != (c == 0.0)) h->structure_dirty = true;   // a block enters or leaves the application: the next setup is a full one
    cij = c;
  });
}

int gmg_block_set_diag_gmg(gmg_block_handle_t h, int i, gmg_handle_t g)
{
  return guarded_b(h, [&] {
    check_block(h, i);
    REQUIRE(g, GMG_ERR_INVALID, "null GMG handle");
    BlockDiag &D = h->diag[i];
    if (D.g && D.g != g) {
      if (D.g->stream == h->eng.stream) D.g->stream = D.g->own_stream;
      if (D.g->attached_to == h) D.g->attached_to = nullptr;
    }
    D = BlockDiag();
    D.kind = GMG_BLOCK_GMG; D.g = g;
    h->touch();
  });
}

int gmg_block_set_diag_krylov_gmg(gmg_block_handle_t h, int i, gmg_handle_t g, int krylov, int m, int restart, int m_add, int flexible,
                                  int side, int maxiter, double atol, double rtol)
{
  return guarded_b(h, [&] {
    check_block(h, i);
    REQUIRE(g, GMG_ERR_INVALID, "null GMG handle");
    REQUIRE(krylov == GMG_KRYLOV_CG || krylov == GMG_KRYLOV_FGMRES || krylov == GMG_KRYLOV_GMRES, GMG_ERR_INVALID,
            "krylov must be GMG_KRYLOV_CG, GMG_KRYLOV_FGMRES or GMG_KRYLOV_GMRES");
    REQUIRE(side == 0 || side == 1, GMG_ERR_INVALID, "side must be 0 (Pr) or 1 (Pl)");
    REQUIRE(krylov != GMG_KRYLOV_FGMRES || side == 0, GMG_ERR_INVALID, "FGMRES takes the GMG as Pr (side 0)");
    REQUIRE(krylov != GMG_KRYLOV_CG || side == 1, GMG_ERR_INVALID, "CG takes the GMG as Pl (side 1)");
    if (krylov != GMG_KRYLOV_CG) REQUIRE(m >= 1 && m_add >= 1, GMG_ERR_INVALID, "bad Krylov basis sizes (m < 1 or m_add < 1)");
    REQUIRE(maxiter >= 0, GMG_ERR_INVALID, "maxiter < 0");
    REQUIRE(g->setup_done, GMG_ERR_INVALID, "the GMG handle of block " + std::to_string(i) + " is not set up");
    REQUIRE(g->lev[0].n == h->bsize(i), GMG_ERR_INVALID, "GMG handle size does not match block " + std::to_string(i));
    BlockDiag &D = h->diag[i];
    if (D.g && D.g != g) {
      if (D.g->stream == h->eng.stream) D.g->stream = D.g->own_stream;
      if (D.g->attached_to == h) D.g->attached_to = nullptr;
    }
    D = BlockDiag();
    D.kind = GMG_BLOCK_KRYLOV_GMG; D.g = g;
    D.krylov = krylov; D.m = m; D.restart = restart != 0; D.m_add = m_add; D.flexible = flexible != 0; D.side = side;
    D.maxiter = maxiter; D.atol = atol; D.rtol = rtol;
    h->touch();
  });
}

int gmg_block_set_diag_solver(gmg_block_handle_t h, int i, int kind, int maxiter, double atol, double rtol)
{
  return guarded_b(h, [&] {
    check_block(h, i);
    REQUIRE(kind == GMG_BLOCK_CG_JACOBI || kind == GMG_BLOCK_LU || kind == GMG_BLOCK_JACOBI, GMG_ERR_INVALID, "bad diagonal solver kind");
    REQUIRE(maxiter >= 0, GMG_ERR_INVALID, "maxiter < 0");
    BlockDiag &D = h->diag[i];
    if (D.g && D.g->stream == h->eng.stream) D.g->stream = D.g->own_stream;
    if (D.g && D.g->attached_to == h) D.g->attached_to = nullptr;   // (the GMG handle is free again: another block handle may take it)
    HostCSR keep;
    const bool had = D.hasM;
    if (had) keep = std::move(D.hM);
    D = BlockDiag();
    if (had) { D.hM = std::move(keep); D.hasM = true; }
    D.kind = kind; D.maxiter = maxiter; D.atol = atol; D.rtol = rtol;
    h->touch();
  });
}

int gmg_block_set_diag_matrix(gmg_block_handle_t h, int i, int64_t n, int64_t nnz, const void *ptr, const void *idx,
                              const double *val, int layout, int index_base, int index_bytes)
{
  return guarded_b(h, [&] {
    check_block(h, i);
    REQUIRE(n == h->bsize(i), GMG_ERR_INVALID, "matrix size does not match the block size");
    h->diag[i].hM = convert_input(n, h->ncols_of(i), nnz, ptr, idx, val, layout, index_base, index_bytes);   // distributed: own rows x [own | ghost]
    h->diag[i].hasM = true;
    h->mdiag[(size_t)i] = BlockMeta();
    h->mdiag[(size_t)i].layout = layout;
    h->touch();
  });
}

int gmg_block_setup(gmg_block_handle_t h)
{
  return guarded_b(h, [&] {
    REQUIRE(h, GMG_ERR_INVALID, "null handle");
    h->setup();
  });
}

// ---- numerical_setup!(ns,A) on a block handle: BlockTriangularSolvers.jl:156-186, BlockDiagonalSolvers.jl:153-163 ---------------
namespace {
// the host copy and the record of block (slot,i,j); GMG_ERR_STATE before the first setup, GMG_ERR_INVALID when it is absent
void block_for_update(gmg_block_handle_t h, int slot, int i, int j, HostCSR *&H, BlockMeta *&meta)
{
  REQUIRE(h, GMG_ERR_INVALID, "null handle");
  REQUIRE(h->was_setup, GMG_ERR_STATE, "gmg_block_update_values before the first gmg_block_setup (numerical_setup missing)");
  REQUIRE(slot == GMG_BLOCK_SLOT_SYSTEM || slot == GMG_BLOCK_SLOT_PRECOND || slot == GMG_BLOCK_SLOT_DIAG_MATRIX, GMG_ERR_INVALID, "bad block slot");
  check_block(h, i);
  if (slot == GMG_BLOCK_SLOT_DIAG_MATRIX) {
    REQUIRE(h->diag[i].hasM, GMG_ERR_INVALID, "diagonal block " + std::to_string(i) + " has no matrix of its own (gmg_block_set_diag_matrix)");
    H = &h->diag[i].hM; meta = &h->mdiag[(size_t)i];
    return;
  }
  check_block(h, j);
  auto &hm = slot == GMG_BLOCK_SLOT_SYSTEM ? h->hsys : h->hpre;
  auto it = hm.find({i, j});
  REQUIRE(it != hm.end(), GMG_ERR_INVALID, "block (" + std::to_string(i) + "," + std::to_string(j) + ") is absent");
  H = &it->second; meta = &(slot == GMG_BLOCK_SLOT_SYSTEM ? h->msys : h->mpre)[{i, j}];
}
} // namespace

int gmg_block_update_values(gmg_block_handle_t h, int slot, int i, int j, const double *val)
{
  return guarded_b(h, [&] {
    HostCSR *H = nullptr;
    BlockMeta *meta = nullptr;
    block_for_update(h, slot, i, j, H, meta);
    REQUIRE(val, GMG_ERR_INVALID, "null values");
    std::memcpy(H->val.data(), val, sizeof(double) * (size_t)H->nnz());   // the 0-based CSR order held by the handle
    meta->dirty = true;
    h->setup_done = false;                                  // structure untouched: gmg_block_setup takes the in-place path when it can
  });
}

int gmg_block_update_values_csc(gmg_block_handle_t h, int slot, int i, int j, const void *colptr, const void *rowidx,
                                const double *val, int index_base, int index_bytes)
{
  return guarded_b(h, [&] {
    HostCSR *Hp = nullptr;
    BlockMeta *meta = nullptr;
    block_for_update(h, slot, i, j, Hp, meta);
    HostCSR &H = *Hp;
    REQUIRE(val, GMG_ERR_INVALID, "null values");
    REQUIRE(meta->layout == GMG_CSC, GMG_ERR_STATE, "gmg_block_update_values_csc: this block was not set in GMG_CSC layout");
    REQUIRE(index_bytes == 4 || index_bytes == 8, GMG_ERR_INVALID, "index_bytes must be 4 or 8");
    REQUIRE(index_base == 0 || index_base == 1, GMG_ERR_INVALID, "index_base must be 0 or 1");
    if (colptr)                                             // a pattern of another size is refused on every call, recorded or not
      REQUIRE(read_index(colptr, 0, index_bytes) == index_base && read_index(colptr, H.ncols, index_bytes) - index_base == H.nnz(), GMG_ERR_INVALID,
              "gmg_block_update_values_csc: the column pointers do not describe the pattern this block was set with");
    std::vector<double> v;
    csc_values_to_csr(v, H.ptr, H.nrows, H.ncols, meta->csc_perm, colptr, rowidx, val, index_base, index_bytes, "gmg_block_update_values_csc", "block");
    H.val.swap(v);
    meta->dirty = true;
    h->setup_done = false;
  });
}

int gmg_block_refresh_diag_solver(gmg_block_handle_t h, int i)
{
  return guarded_b(h, [&] {
    check_block(h, i);
    REQUIRE(h->was_setup, GMG_ERR_STATE, "gmg_block_refresh_diag_solver before the first gmg_block_setup (numerical_setup missing)");
    REQUIRE(h->diag[i].kind != 0, GMG_ERR_STATE, "no solver set for diagonal block " + std::to_string(i));
    h->diag[i].refresh = true;
    h->setup_done = false;
  });
}

int gmg_block_get_setup_info(gmg_block_handle_t h, int *kind, int64_t *blocks_refreshed, int64_t *value_bytes, int64_t *device_bytes)
{
  return guarded_b(h, [&] {
    REQUIRE(h, GMG_ERR_INVALID, "null handle");
    if (kind) *kind = h->info_kind;
    if (blocks_refreshed) *blocks_refreshed = h->info_blocks;
    if (value_bytes) *value_bytes = h->info_value_bytes;
    if (device_bytes) *device_bytes = h->eng.dev_bytes;
  });
}

int gmg_block_precond_apply(gmg_block_handle_t h, const double *b, double *x, int memspace)
{
  return guarded_b(h, [&] {
    check_block_ready(h);
    REQUIRE(b && x, GMG_ERR_INVALID, "null vector");
    const int64_t n = h->N();
    const double *db = h->eng.in_vec(b, n, memspace, h->st_b);
    double *dx = (memspace == GMG_MEM_DEVICE) ? x : h->st_x;
    if (h->kind == GMG_BLOCK_SCHUR && memspace == GMG_MEM_HOST) h->eng.h2d(dx, x, n);   // x on entry is the block solvers' initial guess
    h->precond_apply(dx, db);
    h->eng.out_vec(x, dx, n, memspace);
  });
}

int gmg_block_apply_system(gmg_block_handle_t h, const double *x, double *y, int memspace)
{
  return guarded_b(h, [&] {
    check_block_ready(h);
    REQUIRE(x && y, GMG_ERR_INVALID, "null vector");
    const int64_t n = h->N();
    const double *dx = h->eng.in_vec(x, n, memspace, h->st_b);
    double *dy = (memspace == GMG_MEM_DEVICE) ? y : h->st_x;
    h->sys_apply(dx, dy);
    h->eng.out_vec(y, dy, n, memspace);
  });
}

int gmg_block_fgmres_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int m0, int restart, int m_add,
                           int maxiter, double atol, double rtol, int use_precond, gmg_result *res, double *hist, int hist_cap)
{
  return guarded_b(h, [&] {
    check_block_ready(h);
    REQUIRE(b && x, GMG_ERR_INVALID, "null vector");
    REQUIRE(m0 >= 1 && m_add >= 1 && maxiter >= 0, GMG_ERR_INVALID, "bad FGMRES sizes");
    h->krylov_entry(b, x, memspace, maxiter, atol, rtol, res, hist, hist_cap, [&](int64_t n, const double *db, double *dx, ConvLog &log) {
      KrylovOps ops = h->ops(use_precond != 0);
      return fgmres_core(h->eng, n, n, db, dx, h->fg_V, h->fg_Z, ops, m0, restart != 0, m_add, log);
    });
  });
}

int gmg_block_cg_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int maxiter, double atol, double rtol,
                       int flexible, int use_precond, gmg_result *res, double *hist, int hist_cap)
{
  return guarded_b(h, [&] {
    check_block_ready(h);
    REQUIRE(b && x, GMG_ERR_INVALID, "null vector");
    REQUIRE(maxiter >= 0, GMG_ERR_INVALID, "maxiter < 0");
    h->krylov_entry(b, x, memspace, maxiter, atol, rtol, res, hist, hist_cap, [&](int64_t n, const double *db, double *dx, ConvLog &log) {
      KrylovOps ops = h->ops(use_precond != 0);
      return cg_core(h->eng, n, db, dx, h->kw, h->kp, h->kz, h->kr, ops, flexible != 0, log);
    });
  });
}

int gmg_block_minres_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int maxiter, double atol, double rtol,
                           int use_precond, gmg_result *res, double *hist, int hist_cap)
{
  return guarded_b(h, [&] {
    check_block_ready(h);
    REQUIRE(b && x, GMG_ERR_INVALID, "null vector");
    REQUIRE(maxiter >= 0, GMG_ERR_INVALID, "maxiter < 0");
    h->krylov_entry(b, x, memspace, maxiter, atol, rtol, res, hist, hist_cap, [&](int64_t n, const double *db, double *dx, ConvLog &log) {
      KrylovOps ops = h->ops(use_precond != 0);
      return minres_core(h->eng, n, n, db, dx, h->eng.minres_work(n), h->eng.mr_parts, ops, log);
    });
  });
}

int gmg_block_gmres_solve(gmg_block_handle_t h, const double *b, double *x, int memspace, int m0, int restart, int m_add,
                          int maxiter, double atol, double rtol, int use_precond_right, int use_precond_left, gmg_result *res,
                          double *hist, int hist_cap)
{
  return guarded_b(h, [&] {
    REQUIRE((use_precond_right == 0 || use_precond_right == 1) && (use_precond_left == 0 || use_precond_left == 1), GMG_ERR_INVALID,
            "use_precond_right / use_precond_left must be 0 or 1");
    REQUIRE(!(use_precond_right == 1 && use_precond_left == 1), GMG_ERR_INVALID,
            "the block preconditioner can be Pr or Pl of GMRES, not both (its work vectors are in use)");
    check_block_ready(h);
    REQUIRE(b && x, GMG_ERR_INVALID, "null vector");
    REQUIRE(m0 >= 1 && m_add >= 1 && maxiter >= 0, GMG_ERR_INVALID, "bad GMRES sizes");
    h->krylov_entry(b, x, memspace, maxiter, atol, rtol, res, hist, hist_cap, [&](int64_t n, const double *db, double *dx, ConvLog &log) {
      KrylovOps ops = h->ops(use_precond_right != 0);
      if (use_precond_left) ops.precond_left = [h](double *z, const double *r) { h->precond_apply(z, r); };
      return gmres_core(h->eng, n, n, db, dx, ops, m0, restart != 0, m_add, log);
    });
  });
}

int gmg_block_diag_log(gmg_block_handle_t h, int i, gmg_result *res)
{
  return guarded_b(h, [&] {
    check_block_ready(h);
    check_block(h, i);
    REQUIRE(res, GMG_ERR_INVALID, "null result");
    BlockDiag &D = h->diag[i];
    const ConvLog *L = (D.kind == GMG_BLOCK_GMG) ? &D.g->log : &D.log;
    REQUIRE(!L->residuals.empty(), GMG_ERR_STATE, "this block solver keeps no convergence log");
    const size_t k = std::min<size_t>((size_t)L->num_iters, L->residuals.size() - 1);
    L->export_to(res, nullptr, 0, L->residuals[k]);
  });
}

int gmg_block_diag_stats(gmg_block_handle_t h, int i, int64_t *napplies, int64_t *total_iters)
{
  return guarded_b(h, [&] {
    REQUIRE(h, GMG_ERR_INVALID, "null handle");
    check_block(h, i);
    const BlockDiag &D = h->diag[i];
    REQUIRE(D.kind == GMG_BLOCK_GMG || D.kind == GMG_BLOCK_CG_JACOBI || D.kind == GMG_BLOCK_KRYLOV_GMG, GMG_ERR_STATE,
            "this block solver is not iterative");
    if (napplies) *napplies = D.napplies;
    if (total_iters) *total_iters = D.total_iters;
  });
}

// ---- null space of the block system: the twins of gmg_nullspace_* on the block handle's engine (vectors of length N()) ----------
#define GMG_BLOCK_NS(body) return guarded_b(h, [&] { REQUIRE(h, GMG_ERR_INVALID, "null handle"); ns_single_rank(h->eng); check_block_ready(h); body; })
int gmg_block_nullspace_set(gmg_block_handle_t h, int64_t n, int k, const double *V, int64_t ld, int memspace)
{
  GMG_BLOCK_NS(nsapi_set(h->eng, h->N(), n, k, V, ld, memspace));
}
int gmg_block_nullspace_size(gmg_block_handle_t h, int *k, int64_t *n)
{
  return guarded_b(h, [&] {
    REQUIRE(h && k && n, GMG_ERR_INVALID, "null argument");
    *k = h->eng.ns.k; *n = h->eng.ns.n;
  });
}
int gmg_block_nullspace_get(gmg_block_handle_t h, double *V_out, int64_t ld, int memspace)
{
  return guarded_b(h, [&] { REQUIRE(h, GMG_ERR_INVALID, "null handle"); nsapi_get(h->eng, V_out, ld, memspace); });
}
int gmg_block_nullspace_orthonormalize(gmg_block_handle_t h, int method) { GMG_BLOCK_NS(nsapi_orthonormalize(h->eng, method)); }
int gmg_block_nullspace_project(gmg_block_handle_t h, double *v, double *p, double *alpha_out, int memspace, int subtract)
{
  GMG_BLOCK_NS(nsapi_project(h->eng, v, p, alpha_out, memspace, subtract));
}
int gmg_block_nullspace_make_orthogonal(gmg_block_handle_t h, double *v, double *alpha_out, int memspace)
{
  GMG_BLOCK_NS(nsapi_make_orthogonal(h->eng, v, alpha_out, memspace));
}
int gmg_block_nullspace_reconstruct(gmg_block_handle_t h, double *v, const double *alpha, int memspace)
{
  GMG_BLOCK_NS(nsapi_reconstruct(h->eng, v, alpha, memspace));
}
int gmg_block_nullspace_gram(gmg_block_handle_t h, double *G_out) { GMG_BLOCK_NS(nsapi_gram(h->eng, G_out)); }
int gmg_block_nullspace_dots(gmg_block_handle_t h, const double *v, double *out_k, int memspace)
{
  GMG_BLOCK_NS(nsapi_dots(h->eng, v, out_k, memspace));
}
int gmg_block_nullspace_image_norms(gmg_block_handle_t h, double *out_k)
{
  GMG_BLOCK_NS(nsapi_image_norms(h->eng, out_k, [h](double *x, double *y) { h->sys_apply(x, y); }));
}
#undef GMG_BLOCK_NS
int gmg_block_nullspace_project_guess(gmg_block_handle_t h, int on)
{
  return guarded_b(h, [&] {
    REQUIRE(h, GMG_ERR_INVALID, "null handle");
    if (on) ns_need(h->eng);
    h->eng.ns.project_guess = on != 0;
  });
}

} // extern "C"
