// engine_program.inl -- member functions of Engine<real>, included INSIDE the struct body by engine.hip (one translation unit):
// the layer program on the host: validation (Engine::validate), chained-MLP / stream / pair-compact-lane analyses,
// weight upload, the option table.

  int validate() {
    const int nb = (int)bufs.size();
    auto okb = [&](int b) { return b >= 0 && b < nb; };
    auto fits_w = [&](int off, size_t n) { return (size_t)off + n <= n_weights; };       // n weight entries from offset off (off >= 0)
    for (size_t k = 0; k < ops.size(); ++k) {
      const dqmc_op& op = ops[k];
      const dqmc::OpViews v(op);
      bool ok = true;
      switch (op.kind) {
        case DQMC_OP_FEAT_EN: ok = okb(v.feat_en.dst()) && bufs[v.feat_en.dst()].rows == N && bufs[v.feat_en.dst()].width >= 4 * sys.n_nuc + (v.feat_en.use_spin() ? 1 : 0); break;
        case DQMC_OP_FEAT_EE: {
          const dqmc::FeatEeOp& e = v.feat_ee;
          ok = okb(e.dst()) && bufs[e.dst()].rows == e.n_rows() && bufs[e.dst()].width == 4 && e.table() >= 0 && (size_t)(e.table() + 2 * e.n_rows()) <= n_itable;
          for (int r = 0; r < e.n_rows() && ok; ++r) {          // senders: electron s >= 0, or nucleus -1 - s
            const int rc = h_itable[e.table() + 2 * r], sd = h_itable[e.table() + 2 * r + 1];
            ok = rc >= 0 && rc < N && sd < N && -1 - sd < sys.n_nuc;
          }
          break;
        }
        case DQMC_OP_LINEAR: {
          const dqmc::LinearOp& l = v.lin;
          ok = l.n_pieces() >= 1 && l.n_pieces() <= dqmc::LIN_MAX_PIECES && okb(l.dst());
          for (int p = 0; ok && p < l.n_pieces(); ++p) {
            const int sb = l.src(p), r0 = l.r0(p), K = l.K(p);
            ok = okb(sb) && K >= 1 && pad4(K) <= bufs[sb].width && r0 >= 0 && r0 + (l.bcast(p) ? 1 : l.nrows()) <= bufs[sb].rows;
          }
          if (ok) {
            const dqmc_buf& d = bufs[l.dst()];
            const int ldw = l.ldw(), c0 = l.dst_col0();
            ok = l.dst_r0() >= 0 && l.dst_r0() + l.nrows() <= d.rows && c0 >= 0 && c0 % 4 == 0 && c0 + ldw <= d.width &&
                 l.w() >= 0 && l.w() % 4 == 0 && fits_w(l.w(), (size_t)l.w_rows() * ldw) &&
                 (!l.has_bias() || (l.bias() % 4 == 0 && (size_t)(l.bias() + ldw) <= n_weights)) && l.act() >= 0 && l.act() <= 4;
            if (ok && l.has_residual())
              ok = okb(l.res()) && bufs[l.res()].width >= c0 + ldw && l.res_r0() >= 0 && l.res_r0() + l.nrows() <= bufs[l.res()].rows;
          }
          break;
        }
        case DQMC_OP_SPIN_MEAN: ok = okb(v.spin_mean.src()) && okb(v.spin_mean.dst()) && bufs[v.spin_mean.src()].rows == N && bufs[v.spin_mean.dst()].rows == 2 && bufs[v.spin_mean.src()].width == bufs[v.spin_mean.dst()].width; break;
        case DQMC_OP_ROW_SUM: ok = okb(v.row_sum.src()) && okb(v.row_sum.dst()) && bufs[v.row_sum.dst()].rows == 1 && bufs[v.row_sum.src()].width == bufs[v.row_sum.dst()].width; break;
        case DQMC_OP_CONST: ok = okb(v.cst.dst()) && v.cst.table() >= 0 && fits_w(v.cst.table(), (size_t)bufs[v.cst.dst()].rows * bufs[v.cst.dst()].width); break;
        case DQMC_OP_CONV: case DQMC_OP_EDGE_SUM: {
          const dqmc::EdgeOp& e = v.conv;
          const bool conv = op.kind == DQMC_OP_CONV;
          ok = okb(e.edge()) && (!conv || okb(v.conv.node())) && okb(e.dst()) && bufs[e.dst()].rows == N && e.width() <= bufs[e.edge()].width &&
               (!conv || e.width() <= bufs[v.conv.node()].width) && e.dst_col0() + e.width() <= bufs[e.dst()].width && (size_t)(e.table() + 2 * N * e.S()) <= n_itable;
          for (int q = 0; conv && q < N * e.S() && ok; ++q) {
            const int row = h_itable[e.table() + 2 * q], sd = h_itable[e.table() + 2 * q + 1];
            if (row < 0) continue;
            ok = row < bufs[e.edge()].rows && (sd >= 0 ? sd : -1 - sd) < bufs[v.conv.node()].rows;
          }
          break;
        }
        case DQMC_OP_ORBITALS: {
          const dqmc::OrbitalsOp& o = v.orb;
          if (o.n_env_slot() < 0) { ok = false; break; }
          const size_t ne = (size_t)sys.n_det * N * sys.n_nuc * o.n_env();
          ok = okb(o.src()) && okb(o.dst()) && bufs[o.src()].rows == N && bufs[o.src()].width >= sys.n_det * N && bufs[o.dst()].rows == sys.n_det && bufs[o.dst()].width >= N * N;
          for (int t = 0; ok && t < 4; ++t) ok = o.w(t) >= 0 && fits_w(o.w(t), ne);
          break;
        }
        case DQMC_OP_SLOGDET: ok = okb(v.slogdet.src()) && bufs[v.slogdet.src()].rows == sys.n_det && bufs[v.slogdet.src()].width >= N * N && N <= 64; break;
        case DQMC_OP_FINAL:
          ok = (!v.fin.has_jastrow() || (okb(v.fin.jastrow()) && bufs[v.fin.jastrow()].rows == 1)) && (!v.fin.has_conf_coeff() || (size_t)(v.fin.conf_coeff() + sys.n_det) <= n_weights) &&
               v.fin.alphas() >= 0 && (size_t)(v.fin.alphas() + 2) <= n_weights && v.fin.cusp_kind() >= 0 && v.fin.cusp_kind() <= 2;
          break;
        case DQMC_OP_ATTENTION: {
          const dqmc::AttentionOp& a = v.att;
          const size_t n_kv = (size_t)a.n_const() * a.heads() * a.head_dim();
          ok = a.heads() >= 1 && a.head_dim() >= 1;
          for (int q = 0; ok && q < 4; ++q) ok = okb(a.buf(q)) && bufs[a.buf(q)].rows == N && bufs[a.buf(q)].width >= a.heads() * a.head_dim() && bufs[a.buf(q)].width == bufs[a.q()].width;
          if (ok) ok = a.n_const() >= 0 && (a.n_const() == 0 || (a.const_k() >= 0 && a.const_v() >= 0 && fits_w(a.const_k(), n_kv) && fits_w(a.const_v(), n_kv)));
          if (ok && dqmc::attention_lds_bytes<real>(N, a.head_dim(), a.n_const()) > (size_t)160 * 1024)
            return fail(DQMC_E_UNSUPPORTED, "attention tile set (N, head_dim) exceeds the 160 KiB LDS");
          break;
        }
        default: ok = false;
      }
      if (!ok) return fail(DQMC_E_ARG, "malformed op #" + std::to_string(k) + " kind " + std::to_string(op.kind));
    }
    return DQMC_OK;
  }

  // Row-wise two-layer MLPs (hkext.MLP with one hidden layer: the edge MLPs w / u and the node MLP h of a message-passing
  // layer): LINEAR op k writes a private hidden buffer that exactly one later LINEAR op reads as its single piece, same
  // rows, whole width.  The pair runs as one launch of the chained kernel at k's position, which is legal when nothing
  // between the two ops touches the second layer's output and its residual input is complete before k.
  void analyse_chains() {
    const int no = (int)ops.size(), nb = (int)bufs.size();
    mlp_child.assign(no, -1);
    mlp_skip.assign(no, 0);
    if (!mlp_fuse) return;
    std::vector<int> rd, wr;
    std::vector<std::vector<int>> writers(nb), readers(nb);
    for (int k = 0; k < no; ++k) { op_io(ops[k], rd, wr); for (int b : wr) writers[b].push_back(k); for (int b : rd) readers[b].push_back(k); }
    for (int c = 0; c < no; ++c) {
      const dqmc::LinearOp ch(ops[c]);
      if (ops[c].kind != DQMC_OP_LINEAR || ch.n_pieces() != 1 || ch.bcast(0)) continue;   // one non-broadcast piece
      const int hb = ch.src(0);
      if (writers[hb].size() != 1 || readers[hb].size() != 1) continue;                   // a private hidden buffer
      const int p = writers[hb][0];
      if (p >= c || ops[p].kind != DQMC_OP_LINEAR || mlp_child[p] >= 0 || mlp_skip[p]) continue;
      const dqmc::LinearOp pa(ops[p]);
      if (pa.n_bcast() || pa.has_residual()) continue;                                    // no broadcast pieces, no residual on the hidden layer
      if (pa.dst_r0() != ch.r0(0) || pa.nrows() != ch.nrows() || pa.dst_col0() != 0 || pad4(ch.K(0)) != pa.ldw()) continue;   // same rows, whole width
      if (pa.ldw() > 64 || ch.ldw() > 32) continue;
      if ((pa.act() & 7) > 2 || (ch.act() & 7) > 4) continue;
      bool ok = true;
      if (ch.has_residual()) for (int w : writers[ch.res()]) ok = ok && w < p;            // residual input complete before the pair runs
      for (int m = p + 1; m < c && ok; ++m) {                                             // nobody in between reads or writes the output buffer
        op_io(ops[m], rd, wr);
        for (int b : rd) ok = ok && b != ch.dst();
        for (int b : wr) ok = ok && b != ch.dst();
      }
      if (!ok) continue;
      mlp_child[p] = c;
      mlp_skip[c] = 1;
    }
  }

  // Stream slots of the Laplacian pass.  Edge-stream ops (pair-compact destination) keep slot 1.  Every other op goes, in
  // program order, to a slot whose last op it depends on anyway (directly or through other ops) -- placing it there costs
  // no concurrency -- preferring the main slot, then the slot of its most recent producer, then a free one; only if
  // there is none does it queue behind unrelated work on the main slot.  A chained MLP pair counts as one op.
  void analyse_streams() {
    const int no = (int)ops.size(), nb = (int)bufs.size();
    op_sid.assign(no, 0);
    std::vector<int> rd, wr, rd2, wr2;
    std::vector<std::vector<int>> writers(nb);
    std::vector<std::vector<char>> dep(no, std::vector<char>(no, 0));
    auto io = [&](int k) {
      op_io(ops[k], rd, wr);
      if (mlp_child.size() == (size_t)no && mlp_child[k] >= 0) {
        op_io(ops[mlp_child[k]], rd2, wr2);
        for (int b : rd2) if (b != dqmc::LinearOp(ops[k]).dst()) rd.push_back(b);
        for (int b : wr2) wr.push_back(b);
      }
    };
    int last[4] = {-1, -1, -1, -1};
    for (int k = 0; k < no; ++k) {
      if (mlp_skip.size() == (size_t)no && mlp_skip[k]) {     // rides with its parent (same slot if it has to run on its own)
        op_sid[k] = 0;
        for (int p = 0; p < k; ++p) if (mlp_child[p] == k) op_sid[k] = op_sid[p];
        continue;
      }
      io(k);
      int producer = -1;
      for (int b : rd)
        for (int w : writers[b]) {
          if (w >= k) continue;
          dep[k][w] = 1;
          for (int x = 0; x < w; ++x) if (dep[w][x]) dep[k][x] = 1;
          if (w > producer) producer = w;
        }
      const dqmc_op& o = ops[k];
      const bool edge = (o.kind == DQMC_OP_FEAT_EE && compact[dqmc::FeatEeOp(o).dst()]) || (o.kind == DQMC_OP_LINEAR && compact[dqmc::LinearOp(o).dst()]);
      int sid = 0;
      if (edge) sid = 1;
      else if (o.kind == DQMC_OP_SLOGDET || o.kind == DQMC_OP_FINAL || o.kind == DQMC_OP_ATTENTION) sid = 0;
      else {
        auto eligible = [&](int s_) { return last[s_] < 0 || dep[k][last[s_]]; };
        if (eligible(0)) sid = 0;
        else if (producer >= 0 && op_sid[producer] >= 2 && eligible(op_sid[producer])) sid = op_sid[producer];
        else if (eligible(2)) sid = 2;
        else if (eligible(3)) sid = 3;
        else sid = 0;
      }
      op_sid[k] = sid;
      last[sid] = k;
      for (int b : wr) writers[b].push_back(k);
    }
  }

  // The aggregate buffer of a layer (width padded to 4) is written by its CONV / EDGE_SUM ops, `width` columns each; the LINEAR
  // op that consumes it reads whole groups of 4 columns against zero weight rows.  Where the ops do not fill the padded width
  // (an odd two_particle_dim: 2 x 5 columns of 12) nobody wrote the remaining columns, and a NaN the workspace happened to hold
  // there became NaN x 0 in every output of the layer.  The op that writes the highest columns zeroes them, too.  That is
  // all the padding only if the ops of a destination tile its columns from 0 upwards without a gap, which is what the program
  // compiler emits; any other layout (say, every op aligned to 4 columns) is refused here instead of read unwritten.
  int analyse_pad_columns() {
    pad_end.assign(ops.size(), 0);
    std::vector<std::vector<int>> writers(bufs.size());
    for (size_t k = 0; k < ops.size(); ++k)
      if (ops[k].kind == DQMC_OP_CONV || ops[k].kind == DQMC_OP_EDGE_SUM) writers[dqmc::EdgeOp(ops[k]).dst()].push_back((int)k);
    for (size_t b = 0; b < bufs.size(); ++b) {
      std::vector<int>& w = writers[b];
      if (w.empty()) continue;
      std::stable_sort(w.begin(), w.end(), [&](int x, int y) { return dqmc::EdgeOp(ops[x]).dst_col0() < dqmc::EdgeOp(ops[y]).dst_col0(); });
      int end = 0;
      for (int k : w) {
        const dqmc::EdgeOp c(ops[k]);
        if (c.dst_col0() != end)
          return fail(DQMC_E_UNSUPPORTED, "CONV / EDGE_SUM ops of buffer " + std::to_string(b) + " leave a gap or overlap at column " + std::to_string(end));
        end += c.width();
      }
      if (end < bufs[b].width) pad_end[w.back()] = bufs[b].width;
    }
    return DQMC_OK;
  }

  // Which buffers can carry pair-compact lanes: outputs of FEAT_EE and of row-wise LINEAR ops on them (all
  // pieces compact, none broadcast; residual compact with the same row pairs).  Consumers that understand the
  // compact layout: LINEAR, CONV (edge operand), EDGE_SUM.  Anything else turns the optimisation off.
  void analyse_lanes() {
    const int nb = (int)bufs.size();
    compact.assign(nb, 0);
    pair_rs.assign(nb, std::vector<int>());
    if (!lane_compact) return;
    std::vector<char> full_written(nb, 0);
    bool ok = true;
    auto set_pairs = [&](int b, int row, int rc, int sd) {
      if (pair_rs[b].empty()) pair_rs[b].assign(2 * (size_t)bufs[b].rows, -2);
      int& pr = pair_rs[b][2 * row];
      int& ps = pair_rs[b][2 * row + 1];
      if (pr != -2 && (pr != rc || ps != sd)) ok = false;
      pr = rc; ps = sd;
    };
    for (size_t k = 0; k < ops.size() && ok; ++k) {
      const dqmc::OpViews v(ops[k]);
      // the table's (row, sender) of receiver el must be the row's own pair
      auto own_pairs = [&](const dqmc::EdgeOp& e) {
        for (int q = 0; q < N * e.S() && compact[e.edge()]; ++q) {
          const int row = h_itable[e.table() + 2 * q], snd = h_itable[e.table() + 2 * q + 1];
          if (row >= 0 && (pair_rs[e.edge()][2 * row] != q / e.S() || pair_rs[e.edge()][2 * row + 1] != snd)) ok = false;
        }
      };
      switch (ops[k].kind) {
        case DQMC_OP_FEAT_EE: {
          const dqmc::FeatEeOp& e = v.feat_ee;
          if (full_written[e.dst()]) { ok = false; break; }
          compact[e.dst()] = 1;
          for (int r = 0; r < e.n_rows(); ++r) set_pairs(e.dst(), r, h_itable[e.table() + 2 * r], h_itable[e.table() + 2 * r + 1]);
          break;
        }
        case DQMC_OP_LINEAR: {
          const dqmc::LinearOp& l = v.lin;
          int n_c = 0;
          for (int p = 0; p < l.n_pieces(); ++p) n_c += compact[l.src(p)] ? 1 : 0;
          if (n_c == 0) {
            if (compact[l.dst()] || (l.has_residual() && compact[l.res()])) ok = false;
            full_written[l.dst()] = 1;
            break;
          }
          if (n_c != l.n_pieces() || full_written[l.dst()]) { ok = false; break; }
          compact[l.dst()] = 1;
          // every source row (pieces and residual) of a destination row carries the same pair
          auto pair_is = [&](int b, int row, int rc, int sd) { return !pair_rs[b].empty() && pair_rs[b][2 * row] == rc && pair_rs[b][2 * row + 1] == sd; };
          for (int rr = 0; rr < l.nrows() && ok; ++rr) {
            const int sb0 = l.src(0), r00 = l.r0(0);
            if (l.bcast(0) || pair_rs[sb0].empty()) { ok = false; break; }
            const int rc = pair_rs[sb0][2 * (r00 + rr)], sd = pair_rs[sb0][2 * (r00 + rr) + 1];
            for (int p = 1; p < l.n_pieces(); ++p)
              if (l.bcast(p) || !pair_is(l.src(p), l.r0(p) + rr, rc, sd)) ok = false;
            if (l.has_residual() && (!compact[l.res()] || !pair_is(l.res(), l.res_r0() + rr, rc, sd))) ok = false;
            set_pairs(l.dst(), l.dst_r0() + rr, rc, sd);
          }
          break;
        }
        case DQMC_OP_CONV:
          if (compact[v.conv.node()] || compact[v.conv.dst()]) ok = false;
          full_written[v.conv.dst()] = 1;
          own_pairs(v.conv);
          break;
        case DQMC_OP_EDGE_SUM:
          if (compact[v.edge_sum.dst()]) ok = false;
          full_written[v.edge_sum.dst()] = 1;
          own_pairs(v.edge_sum);
          break;
        case DQMC_OP_FEAT_EN: full_written[v.feat_en.dst()] = 1; break;
        case DQMC_OP_CONST: full_written[v.cst.dst()] = 1; break;
        case DQMC_OP_SPIN_MEAN: if (compact[v.spin_mean.src()]) ok = false; full_written[v.spin_mean.dst()] = 1; break;
        case DQMC_OP_ROW_SUM: if (compact[v.row_sum.src()]) ok = false; full_written[v.row_sum.dst()] = 1; break;
        case DQMC_OP_ORBITALS: if (compact[v.orb.src()]) ok = false; full_written[v.orb.dst()] = 1; break;
        case DQMC_OP_SLOGDET: if (compact[v.slogdet.src()]) ok = false; break;
        case DQMC_OP_FINAL: if (v.fin.has_jastrow() && compact[v.fin.jastrow()]) ok = false; break;
        case DQMC_OP_ATTENTION:
          for (int q = 0; q < 3; ++q) if (compact[v.att.buf(q)]) ok = false;
          full_written[v.att.dst()] = 1;
          break;
        default: break;
      }
    }
    for (int b = 0; b < nb && ok; ++b)
      if (compact[b]) for (int v : pair_rs[b]) if (v == -2) ok = false;   // every row of a compact buffer has a pair
    if (!ok) { compact.assign(nb, 0); pair_rs.assign(nb, std::vector<int>()); }
  }
  // lanes of buffer b in an evaluation with TP lanes
  int lanes_of(int b, int TP) const { return (TP > 1 && compact[b]) ? dqmc::PAIR_LANES : TP; }

  int set_weights(const double* w, size_t n) override {
    if (n != n_weights) return fail(DQMC_E_ARG, "weight buffer length differs from the one given at creation");
    ++graph_epoch;
    dev_ahead = false;                       // (engine_optim.inl: the host copies below are the newest again)
    nuc_fresh = false;                       // (engine_nuc.inl: the constants below were folded on the host)
    if (d_w64) HIP_TRY(hipMemcpyAsync(d_w64, w, sizeof(double) * n, hipMemcpyHostToDevice, st));
    wtmp.resize(n);
    for (size_t k = 0; k < n; ++k) wtmp[k] = (real)w[k];
    if (sizeof(real) == 4) {
      w64_h.assign(w, w + n);
      if (twin) { const int rc = twin->set_weights(w, n); if (rc) return rc; }
    }
    HIP_TRY(hipMemcpyAsync(d_w, wtmp.data(), sizeof(real) * n, hipMemcpyHostToDevice, st));
    HIP_TRY(hipStreamSynchronize(st));
    const int rc_t = pack_spec_tape();
    if (rc_t) return rc_t;
    if (fused_n_ops > 0) return pack_fused_weights();
    return DQMC_OK;
  }
  // FNV-1a over the integers that define the program's structure (deepqmc_amd/codegen/substep.py: program_hash computes the
  // same value when it generates a plan-specialised kernel)
  uint64_t program_hash() const {
    uint64_t h = 0xcbf29ce484222325ull;
    auto mix = [&](int32_t v) {
      for (int k = 0; k < 4; ++k) { h = (h ^ (uint64_t)((uint32_t)v >> (8 * k) & 0xffu)) * 0x100000001b3ull; }
    };
    mix(sys.n_up); mix(sys.n_down); mix(sys.n_nuc); mix(sys.n_det); mix((int32_t)bufs.size()); mix((int32_t)ops.size()); mix((int32_t)n_itable);
    for (const auto& b : bufs) { mix(b.rows); mix(b.width); }
    for (const auto& o : ops) {
      mix(o.kind);
      for (int k = 0; k < dqmc::OP_N_SLOTS; ++k) mix(o.i[k]);
      for (int k = 0; k < dqmc::OP_N_FSLOTS; ++k) { int32_t bits; memcpy(&bits, &o.f[k], 4); mix(bits); }
    }
    for (int32_t v : h_itable) mix(v);
    return h;
  }
  int pack_spec_tape() {
    if constexpr (sizeof(real) == 4) {
      if (!spec_k) return DQMC_OK;
      std::vector<uint32_t> tape((size_t)spec_k->tape_bytes / 4);
      dqmc::spec_pack_tape(*spec_k, reinterpret_cast<const float*>(wtmp.data()), tape.data());
      { const int rc = d_tape.reserve((size_t)spec_k->tape_bytes / 4, st); if (rc) return rc; }
      HIP_TRY(hipMemcpyAsync(d_tape, tape.data(), (size_t)spec_k->tape_bytes, hipMemcpyHostToDevice, st));
      HIP_TRY(hipStreamSynchronize(st));
    }
    return DQMC_OK;
  }
  // ---- fused value-only evaluation (kernel_fused2.hip) ----------------------------------
  // Ops [0, fused_n_ops) (everything up to and including ORBITALS) run in one kernel on a tile
  // of WT walkers with LDS-resident buffers; buffers read by later ops stay in the workspace.
  int option(const char* name, int value) override {
    const std::string s(name);
    if (s.rfind("twin.", 0) == 0) {            // an option of the float64 refinement twin (applied when it is created, too)
      twin_opts.emplace_back(s.substr(5), value);
      return twin ? twin->option(s.c_str() + 5, value) : DQMC_OK;
    }
    ++graph_epoch;                             // (any switch may change what a captured pass would launch)
    if (s == "pass_graph") { pass_graph = value; if (!value) drop_graphs(); if (twin) twin->option("pass_graph", value); twin_opts.emplace_back(s, value); return DQMC_OK; }
    if (s == "fused") { fused_enabled = value; return DQMC_OK; }
    if (s == "fused_wt") { fused_wt_req = value; return build_fused_plan(); }
    if (s == "fused_occ") { fused_occ_req = value; return DQMC_OK; }
    if (s == "attention_mfma") { attention_mfma = value; return DQMC_OK; }
    if (s == "attention_ncb") { attention_ncb = value; return DQMC_OK; }
    if (s == "attention_split") { attention_split = value; return DQMC_OK; }
    if (s == "attention_reverse") { if (value != 0 && value != 1) return fail(DQMC_E_ARG, "attention_reverse must be 0 or 1"); attention_reverse = value; return DQMC_OK; }
    if (s == "nuclear_reverse") {
      if (value != 0 && value != 1) return fail(DQMC_E_ARG, "nuclear_reverse must be 0 or 1");
      if (value && !nuc_set) return fail(DQMC_E_ARG, "nuclear_reverse needs a registered nuclear stream (dqmc_set_nuclear_stream)");
      nuclear_reverse = value;
      return DQMC_OK;
    }
    if (s == "nuclear_coords") {
      if (value != 0 && value != 1) return fail(DQMC_E_ARG, "nuclear_coords must be 0 or 1");
      if (value && (!nuc_set || !nuclear_reverse))
        return fail(DQMC_E_ARG, "nuclear_coords needs a registered nuclear stream (dqmc_set_nuclear_stream) and nuclear_reverse 1");
      nuclear_coords = value;
      return DQMC_OK;
    }
    if (s == "nuclear_params") {
      if (value != 0 && value != 1) return fail(DQMC_E_ARG, "nuclear_params must be 0 or 1");
      if (value && (!nuc_set || !nuclear_reverse))
        return fail(DQMC_E_ARG, "nuclear_params needs a registered nuclear stream (dqmc_set_nuclear_stream) and nuclear_reverse 1");
      nuclear_params = value;
      return DQMC_OK;
    }
    if (s == "ws_budget_mb") { if (value < 1) return fail(DQMC_E_ARG, "ws_budget_mb must be positive"); ws_budget = (size_t)value << 20; return DQMC_OK; }
    if (s == "slogdet_mfma") { slogdet_mfma = value; return DQMC_OK; }
    if (s == "lane_compact") { lane_compact = value != 0; analyse_lanes(); last_B = 0; return DQMC_OK; }
    if (s == "linear_f64_split") { linear_f64_split = value; return DQMC_OK; }
    if (s == "linear_bkx") { linear_bkx = value; return DQMC_OK; }      // (kernel selection of kernel_linear.hip, this context only)
    if (s == "mlp_fuse") { mlp_fuse = value; analyse_chains(); return DQMC_OK; }
    if (s == "no_twin") { if (value && twin) return fail(DQMC_E_ARG, "no_twin must be set before the first local-energy call creates the twin"); no_twin = value; return DQMC_OK; }
    if (s == "fused_substep") { fused_substep = value; return DQMC_OK; }
    if (s == "fused_spec") { fused_spec = value; return DQMC_OK; }
    if (s == "split_bcast") { split_bcast = value; return DQMC_OK; }
    if (s == "dual_stream") { dual_stream = value; return DQMC_OK; }
    if (s == "multi_stream") { multi_stream = value; return DQMC_OK; }
    if (s == "fused_prio") { fused_prio = value; return DQMC_OK; }
    if (s == "fused_lean") { fused_lean = value; return build_fused_plan(); }
    if (s == "fused_bf") { fused_bf = value; return build_fused_plan(); }
    if (s == "linear_bf") { linear_bf = value; return DQMC_OK; }      // (kernel selection of kernel_linear.hip, this context only)
    if (s == "fused_wg_per_cu") {
      if (value < 4 || value > 6) return fail(DQMC_E_ARG, "fused_wg_per_cu must be 4, 5 or 6");
      fused2_lds_quarter = (size_t)160 * 1024 / value;
      return build_fused_plan();
    }
    if (s == "refine") { refine = value; return DQMC_OK; }
    if (s == "twin_full_budget") { twin_full_budget = value; if (twin) twin->option("ws_budget_mb", (int)((value ? ws_budget : ws_budget / 2) >> 20)); return DQMC_OK; }
    if (s == "refine_sample") { if (value < 2) return fail(DQMC_E_ARG, "refine_sample must be >= 2"); refine_sample = value; calls_since_probe = -1; return DQMC_OK; }
    if (s == "refine_probe") { if (value < 0) return fail(DQMC_E_ARG, "refine_probe must be >= 0"); refine_probe = value; calls_since_probe = -1; return DQMC_OK; }
    if (s == "refine_miss_e9") { if (value < 1) return fail(DQMC_E_ARG, "refine_miss_e9 must be >= 1"); refine_miss = 1e-9 * value; calls_since_probe = -1; return DQMC_OK; }
    if (s == "refine_target_e7") { if (value < 1) return fail(DQMC_E_ARG, "refine_target_e7 must be >= 1"); refine_target = 1e-7 * value; calls_since_probe = -1; return DQMC_OK; }
    if (s == "refine_direct_calls") { if (value < 0) return fail(DQMC_E_ARG, "refine_direct_calls must be >= 0"); direct.calls = value; return DQMC_OK; }
    if (s == "refine_direct_backoff") { if (value < 0 || value > 16) return fail(DQMC_E_ARG, "refine_direct_backoff must be in [0, 16]"); direct.backoff = value; return DQMC_OK; }
    if (s == "refine_direct_pct") { if (value < 1 || value > 100) return fail(DQMC_E_ARG, "refine_direct_pct must be 1..100"); direct.enter = 0.01 * value; if (direct.exit > direct.enter) direct.exit = direct.enter; return DQMC_OK; }
    if (s == "refine_direct_exit_pct") { if (value < 0 || value > 100) return fail(DQMC_E_ARG, "refine_direct_exit_pct must be 0..100"); direct.exit = 0.01 * value; if (direct.exit > direct.enter) direct.enter = direct.exit; return DQMC_OK; }
    if (s == "refine_thresh") { if (value < 0) return fail(DQMC_E_ARG, "refine_thresh must be >= 0"); refine_thresh = (double)value; return DQMC_OK; }
    if (s == "fused_sched_kb") { fused_sched_budget = (size_t)value * 1024; return build_fused_plan(); }
    if (s == "fused_print") {   // plan summary on stderr (tuning aid)
      fprintf(stderr, "[dqmc] fused plan: WT=%d lds=%zu B; %d fused ops, %d levels\n", fused2_WT, fused2_lds, fused_n_ops,
              fused_n_ops ? f_level[fused_n_ops - 1] + 1 : 0);
      if (value >= 2)        // one line per descriptor of every wave list: kind, scheduled op, its op kind, row blocks, quads of k-steps
        for (size_t w = 0; w < plan_lists.size(); ++w)
          for (size_t k = 0; k < plan_lists[w].size(); ++k) {
            const dqmc::FDesc& d = plan_lists[w][k];
            int nq = 0;
            for (int p = 0; p < d.n_pieces; ++p) nq += d.a_nq[p];
            fprintf(stderr, "[dqmc] wave %zu desc %zu kind %d op %d opkind %d ma %d row0 %d col0 %d quads %d ldw %d\n", w, k, d.kind, d.op,
                    d.kind == 2 ? 0 : ops[f_order[d.op]].kind, d.ma, d.row0, d.col0, nq, d.ldw);
          }
      return DQMC_OK;
    }
    if (s == "ecp_mixed") { ecp_mixed_on = value; return DQMC_OK; }
    if (s == "ecp_heavy_e6") { if (value < 0) return fail(DQMC_E_ARG, "ecp_heavy_e6 must be >= 0"); ecp_w_heavy = 1e-6 * value; return DQMC_OK; }
    if (s == "ecp_dlog_floor_e6") { if (value < 0) return fail(DQMC_E_ARG, "ecp_dlog_floor_e6 must be >= 0"); ecp_dlog_floor = 1e-6 * value; return DQMC_OK; }
    if (s == "ecp_skip_e12") { if (value < 0) return fail(DQMC_E_ARG, "ecp_skip_e12 must be >= 0"); ecp_w_skip = 1e-12 * value; return DQMC_OK; }
    if (s == "ecp_max_cfg") { if (value < 1) return fail(DQMC_E_ARG, "ecp_max_cfg must be positive"); ecp_max_cfg = (size_t)value; return DQMC_OK; }
    if (s == "fused_sched") { fused_sched_mode = value; return build_fused_plan(); }
    if (s == "fused_dbg") {
      fused_dbg = value;
      if (value && !d_prof) {
        const int rc = d_prof.assign(9 * ops.size() + 80 + 1024 + 2 * 8192);
        if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d_prof, 0, sizeof(long long) * d_prof.cap, st));
      }
      return DQMC_OK;
    }
    if (s == "fused_lds_kb") { fused2_lds_budget = (size_t)value * 1024; return build_fused_plan(); }
    return fail(DQMC_E_ARG, "unknown option " + s);
  }

  // LDS placement of the buffers for a tile of WT walkers: first-fit over live intervals.
  // Buffers read / written by an op (buffer granularity; partial writers of one buffer touch
  // disjoint row or column ranges by construction of the program).
