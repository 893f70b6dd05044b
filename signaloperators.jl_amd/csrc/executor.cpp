// Executor: buffer allocation and table upload (finalize), multi-stream lanes, launches, HIP-graph
// replay, so_plan_set_array, statistics.
#include "plan_impl.h"

namespace so {

// May the kernels read this carrier's array 16 bytes at a time (LDS-DMA, vector loads)?  Rows only need their element's
// natural alignment: the memory pipeline takes a 16-byte access at any 8-byte address -- LDS-DMA included (measured:
// a [channels x frames] device tensor with an ODD number of frames, every second row 8 bytes off, used to send every chunk
// of K3 and of the fused kernel down the general staging path: 8 channels x 12 500 001 frames 5.06 ms, now 0.70; same
// values); Float32 rows likewise from any 4-byte address (8 ch x 12 500 001: 5.4 -> 0.77 ms).
static inline int carrier_vec_ok(const DCarrier& c, int64_t V) {
    if (!std::getenv("SIGOPS_STRICT_ALIGN")) return (uintptr_t)c.base % (c.dtype == SO_F64 ? 8 : 4) == 0;
    return ((uintptr_t)c.base % 16 == 0) && (c.cstride % V == 0);
}

// ---------------------------------------------------------------------------
// Plan tables go up in pieces of 16 KB: the runtime sets its staging path for pageable copies of 32 KB and more up on the
// first such copy of the PROCESS -- 6 ms, measured, which the 66 KB tap table of a first one-shot sink paid (a host that has
// already copied its signal to the device has paid it; one whose data was produced on the device has not).  Small copies go
// another way.  Tables of more than a megabyte are not chopped up.
static hipError_t h2d_small(void* dst, const void* src, size_t bytes) {
    constexpr size_t kPiece = 16 * 1024;
    if (bytes < 2 * kPiece || bytes > (1u << 20)) return hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice);
    for (size_t off = 0; off < bytes; off += kPiece) {
        const hipError_t e = hipMemcpy((char*)dst + off, (const char*)src + off, std::min(kPiece, bytes - off), hipMemcpyHostToDevice);
        if (e != hipSuccess) return e;
    }
    return hipSuccess;
}

// ---------------------------------------------------------------------------
// finalize's tables: the pointwise steps' pieces, programs and leaves, the look-up tables, and per stage what its kernels
// read -- straight from the stages' *_host vectors (std::vector<Stage> moves while the planner adds stages: no pointers kept).
static void upload_tables(Plan* P) {
    std::vector<Buf>& bufs = P->bufs;
    auto up = [&](int buf, const auto& v, size_t at = 0) {  // vector v into plan buffer `buf`, from byte `at` on
        HIPCHECK(h2d_small((char*)bufs[buf].d + at, v.data(), v.size() * sizeof(*v.data())));
    };
    auto alloc_up = [](auto*& d, const auto& v) {  // a table with an allocation of its own, where there is one
        if (v.empty()) return;
        HIPCHECK(hipMalloc(&d, v.size() * sizeof(*v.data())));
        HIPCHECK(h2d_small(d, v.data(), v.size() * sizeof(*v.data())));
    };
    alloc_up(P->d_pieces, P->pieces);
    alloc_up(P->d_ops, P->ops);
    alloc_up(P->d_leaves, P->leaves);
    for (auto& T : P->tables)  // SO_EOP_INTERP: the only copy of a table the plan ever makes
        HIPCHECK(h2d_small(bufs[T.buf].d, T.src, T.ndoubles * 8));
    for (auto& S : P->stages) {
        if (S.need <= 0) continue;
        if (S.kind == ST_SOS && S.qmat_buf >= 0) up(S.qmat_buf, S.qmat_host);
        if (S.kind == ST_SOS && S.rsos_src >= 0) {
            up(S.rsos_mats_buf, S.rsos_mats_host);
            if (S.rsos_jrel_buf >= 0) up(S.rsos_jrel_buf, S.rsos_jrel_host);
            if (S.rsos_tab_buf >= 0) {
                up(S.rsos_tab_buf, S.rsos_tab_host);
                up(S.rsos_jend_buf, S.rsos_jend_host);
            }
        }
        if (S.kind == ST_SOS && S.onepass) up(S.one_tabs_buf, S.one_tabs_host);
        if (S.kind == ST_RESAMPLE && S.rs_jrel_buf >= 0 && S.rs_nf_buf >= 0) {
            up(S.rs_jrel_buf, S.rs_jrel_host);
            HIPCHECK(hipMemset(bufs[S.rs_nf_buf].d, 0, 64));  // (the list's count: k_rs_fixup leaves it at zero again)
        }
        if (S.kind == ST_RESAMPLE) {
            up(S.pfb_buf, S.pfb_host);
            up(S.dpfb_buf, S.dpfb_host);
            if (S.wtab_buf >= 0) up(S.wtab_buf, S.wtab_host);
            if (S.tiled) {
                up(S.pfbt_buf, S.pfbt_host);
                up(S.dpfbt_buf, S.dpfbt_host);
            }
            if (S.fix_buf >= 0) up(S.fix_buf, S.fix_host);
            if (S.periodic || S.rows) {
                up(S.tab_buf, S.tab_host);
                up(S.jend_buf, S.jend_host);
            }
            if (S.rows && !S.mtab_host.empty()) {
                up(S.mtab_buf, S.mtab_host);
                up(S.mjend_buf, S.mjend_host);
            }
        } else if (S.kind == ST_SOS && S.mpow_buf >= 0) {
            for (size_t gi = 0; gi < S.xs_mats_host.size() && S.xs_mats_buf >= 0; ++gi) up(S.xs_mats_buf, S.xs_mats_host[gi], gi * 2 * 16 * 16 * 8);
            for (size_t gi = 0; gi < S.mpow_host.size(); ++gi) up(S.mpow_buf, S.mpow_host[gi], gi * S.mpow_stride() * 8);
        }
    }
}

// The name a stage's step goes by in so_plan_step_info: the kernel that does its work.
static const char* stage_step_name(const Stage& S) {
    switch (S.kind) {
    case ST_SOS: return S.rsos_src >= 0 ? "k_rsos" : S.sg.exact ? "k_sos_exact" : "k_sos";
    case ST_RESAMPLE:
        if (S.periodic) return "k_resample_periodic";
        if (S.rows) return "k_resample_rows";
        if (S.tiled) return S.arbk ? "k_resample_arb" : S.rt.pair ? "k_resample_tiled2" : "k_resample_tiled";
        return "k_resample";
    case ST_SAMPLEAT: return S.sa_kind == 1 ? "k_sample_at_cubic" : S.sa_kind == 2 ? "k_sample_at_sinc" : "k_sample_at";
    }
    for (const StageNodeKind& k : kStageNodes)
        if (k.stage == S.kind) return k.step;
    return "k_sumsq";
}

// Algorithmic bytes of a stage: the samples it reads in the type they have WHERE THEY LIE (a Float32 array under a Float64
// map is 4 bytes a sample, whatever the node's promoted type) plus the samples it writes in the type of the buffer they go
// to (a Float64 stage that rounds into the Float32 result itself writes 4).
static int64_t stage_step_bytes(const Plan* P, int sid) {
    const Stage& S = P->stages[sid];
    const Node& N = P->nodes[S.node];
    const int64_t esz = (int64_t)dsize(N.dtype);
    const int64_t osz = (sid == P->alias_stage && P->alias_narrow) ? (int64_t)dsize(P->out.dtype) : esz;
    auto src_esz = [&](const Stage& R) -> int64_t {  // a resampler's source: carrier 0's array / buffer, else its child
        if (!R.carriers.empty()) return (int64_t)dsize(R.carriers[0].dtype);
        const std::vector<int>& kids = P->nodes[R.node].kids;
        return !kids.empty() && kids[0] >= 0 ? (int64_t)dsize(P->nodes[kids[0]].dtype) : esz;
    };
    auto kid_esz = [&](int k) { return (int64_t)dsize(P->nodes[N.kids[k]].dtype); };
    switch (S.kind) {
    case ST_SOS:
        if (S.rsos_src >= 0)  // (arr2: a second array read)
            return (S.rs.n_in * src_esz(P->stages[S.rsos_src]) * (S.rs.arr2 ? 2 : 1) + S.rs.n_out * osz) * S.rs.nch;
        return (S.need - S.base) * S.sg.nch * (esz + osz);
    case ST_RESAMPLE:  // (arr2: a second array of the source's type read)
        return (S.rg.n_in * (src_esz(S) + (S.rp.arr2 ? src_esz(S) : 0)) + S.rg.n_out * osz) * S.rg.nch;
    case ST_SAMPLEAT: {  // per frame: a position read, the table samples of its support read where they lie (2, 4 or K), a Float64 written
        const int64_t taps = S.sa_kind == 1 ? 4 : S.sa_kind == 2 ? N.nd.i2 : 2;
        return (S.need - S.base) * ((int64_t)P->nodes[N.kids[1]].nch * 8 + (int64_t)N.nch * (taps * kid_esz(0) + 8));
    }
    case ST_COMB:  // per sample: one read where x lies, one Float64 written
        return (S.need - S.base) * (int64_t)N.nch * (kid_esz(0) + 8);
    case ST_CUMSUM:  // per sample: two reads where x lies (the totals' pass and the scan's), one Float64 written
        return (S.need - S.base) * (int64_t)N.nch * (2 * kid_esz(0) + 8);
    case ST_MOVING:  // the frames read where x lies (the long form's second and third reads and the tile halos left out), one sample of x's type written
        return (S.in_frames + (S.need - S.base)) * (int64_t)N.nch * esz;
    case ST_MOVRANK:  // the frames read where x lies (the tile halos left out), one sample of x's type written
        return (S.in_frames + (S.need - S.base)) * (int64_t)N.nch * esz;
    case ST_MOVSUM:  // the frames read where x lies (the long form's further reads, the tile halos and lead-ins left out), one Float64 written
        return (S.in_frames * kid_esz(0) + (S.need - S.base) * 8) * (int64_t)N.nch;
    case ST_RECUR: {  // per sample: b read twice where it lies (the totals' pass and the scan's), a row of a twice as Float64, one Float64 written
        const bool row = N.kids.size() == 2;
        const int64_t a_rows = !row ? 0 : S.side[0].pitch == 0 ? 1 : N.nch;
        return (S.need - S.base) * ((int64_t)N.nch * (2 * kid_esz(row ? 1 : 0) + 8) + a_rows * 16);
    }
    case ST_RECUR2: {  // per sample: b read twice where it lies, each row of a1 and of a2 twice as Float64, one Float64 written
        const bool row = N.kids.size() == 3;
        int64_t a_rows = 0;
        for (int w = 0; row && w < 2; ++w) a_rows += S.side[w].pitch == 0 ? 1 : N.nch;
        return (S.need - S.base) * ((int64_t)N.nch * (2 * kid_esz(row ? 2 : 0) + 8) + a_rows * 16);
    }
    default: return (S.need - S.base) * N.nch * esz;
    }
}

void Plan::finalize() {
    // size stage output buffers now that every need is known
    for (size_t si = 0; si < stages.size(); ++si) {
        Stage& S = stages[si];
        if (S.out_buf >= 0 && ((int)si == alias_stage || S.win_off >= 0)) {
            bufs[S.out_buf].external = true;  // the kernel writes the final output directly
            bufs[S.out_buf].bytes = 0;
            continue;
        }
        if (S.out_buf >= 0 && (S.fused_away || S.norm_direct)) {  // (its consumer computes it on the fly: k_rsos; Normpower reading an array in place)
            bufs[S.out_buf].frames = 0;
            bufs[S.out_buf].bytes = 64;
            continue;
        }
        if (S.out_buf >= 0) {
            Buf& b = bufs[S.out_buf];
            b.frames = S.need - S.base;
            b.pitch = std::max<int64_t>(64, (S.need - S.base + 63) / 64 * 64);
            b.bytes = (size_t)b.pitch * (size_t)std::max(b.nch, 1) * dsize(b.dtype);
        }
    }
    // host array leaves get a device copy (the leaves of pointwise programs, the carriers of fused
    // resampler sources and the direct sources of stages go through the same validation)
    auto stage_host_array = [&](int an) {
        if (an < 0) return;
        const so_node_t& nd = nodes[an].nd;
        if (nd.i0 || array_buf.count(an)) return;  // device-resident, or already staged
        if (nd.s0 < 0 || nd.s1 < 0) fail(SO_ERR_UNSUPPORTED, "negative strides on host arrays are not supported");
        const size_t extent = nd.l0 > 0 ? (size_t)((nd.l0 - 1) * nd.s0 + (int64_t)(nd.nch - 1) * nd.s1 + 1) : 0;
        const int b = raw_buf(extent * dsize(nd.dtype));
        array_buf[an] = b;
        host_leaves.push_back(HostLeaf{an, nd.p0, extent * dsize(nd.dtype), b});
    };
    for (size_t i = 0; i < leaves.size(); ++i) stage_host_array(leaf_array_node[i]);
    for (auto& S : stages) {
        for (auto& c : S.carriers) {
            stage_host_array(c.array_node);
            if (car_has_arr2(c)) stage_host_array(c.array_node2);
        }
        stage_host_array(S.in_array_node);
        for (auto& sd : S.side) stage_host_array(sd.array_node);
    }
    if (!out.is_device && out.nframes > 0) {
        Buf b;
        b.frames = out.nframes;
        b.pitch = out.nframes;
        b.nch = out.nch;
        b.dtype = out.dtype;
        b.bytes = (size_t)out.nframes * out.nch * dsize(out.dtype);
        bufs.push_back(b);
        out_stage_buf = (int)bufs.size() - 1;
    }
    // allocate
    const bool dbg_t = std::getenv("SIGOPS_DEBUG_PLAN") != nullptr;
    const auto tf0 = std::chrono::steady_clock::now();
    int64_t scratch = 0;
    int nalloc = 0;
    for (auto& b : bufs) {
        if (b.external) continue;
        HIPCHECK(hipMalloc(&b.d, std::max<size_t>(b.bytes, 64)));
        scratch += (int64_t)b.bytes;
        ++nalloc;
    }
    stats.scratch_bytes = scratch;
    if (dbg_t)
        std::fprintf(stderr, "[sigops] finalize: %d hipMalloc calls, %lld bytes: %.3f ms\n", nalloc, (long long)scratch,
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count());
    if (out_alias_buf >= 0 && !out.is_device) {
        bufs[out_alias_buf].d = bufs[out_stage_buf].d;
        bufs[out_alias_buf].pitch = bufs[out_stage_buf].pitch;
    }
    // patch leaves
    for (size_t i = 0; i < leaves.size(); ++i) {
        DLeaf& L = leaves[i];
        int an = leaf_array_node[i];
        if (an >= 0) {
            L.base = nodes[an].nd.i0 ? array_ptr[an] : bufs[array_buf[an]].d;
        } else if (L.buf >= 0) {
            L.base = bufs[L.buf].d;
            if (L.cstride == -1) L.cstride = bufs[L.buf].pitch;
            L.df -= bufs[L.buf].frame0;  // (stage buffers that start at a later frame: once, here)
        }
    }
    // scalar leaves of a Normpower's rms: patched on the device by the launch that computes it (RmsPatch)
    for (auto& S : stages) {
        if (S.kind != ST_NORM || S.rms_buf < 0 || std::getenv("SIGOPS_NO_RMSPATCH")) continue;
        S.rms_leaves.clear();
        for (size_t i = 0; i < leaves.size(); ++i)
            if (leaves[i].buf == S.rms_buf && leaf_array_node[i] < 0) S.rms_leaves.push_back((int)i);
        if (S.rms_leaves.size() > 8) S.rms_leaves.clear();
        for (int i : S.rms_leaves) leaves[(size_t)i].flag = 1;
    }
    for (auto& S : stages) {
        if (S.carriers.empty()) continue;
        for (auto& c : S.carriers) {
            if (c.array_node >= 0) {
                const so_node_t& nd = nodes[c.array_node].nd;
                if (!nd.i0 && !array_buf.count(c.array_node)) fail(SO_ERR_RUNTIME, "internal: carrier array without device copy");
                c.base = nd.i0 ? array_ptr[c.array_node] : bufs[array_buf[c.array_node]].d;
            } else if (c.buf >= 0) {
                c.base = bufs[c.buf].d;
                if (c.cstride == -1) c.cstride = bufs[c.buf].pitch;
                c.df -= bufs[c.buf].frame0;
            } else {
                c.base = nullptr;  // generated piece
                c.cstride = 0;
            }
            const int64_t V = 16 / (int64_t)dsize(c.dtype);
            c.vec_ok = carrier_vec_ok(c, V);
            if (car_has_arr2(c)) {  // the step's second array (a caller's: match_carrier)
                const so_node_t& nd = nodes[c.array_node2].nd;
                if (!nd.i0 && !array_buf.count(c.array_node2)) fail(SO_ERR_RUNTIME, "internal: carrier array without device copy");
                c.base2 = nd.i0 ? array_ptr[c.array_node2] : bufs[array_buf[c.array_node2]].d;
                c.vec_ok2 = (uintptr_t)c.base2 % (c.dtype2 == SO_F64 ? 8 : 4) == 0;
            } else {
                c.base2 = nullptr;
                c.array_node2 = c.buf2 = -1;
            }
        }
        if (std::getenv("SIGOPS_DEBUG_PLAN"))
            for (auto& c : S.carriers)
                std::fprintf(stderr, "[sigops] carrier [%lld,%lld) base=%p cstride=%lld df=%lld dtype=%d vec_ok=%d nsteps=%d frame_len=%d depth=%d\n",
                             (long long)c.a, (long long)c.b, c.base, (long long)c.cstride, (long long)c.df, c.dtype, c.vec_ok, c.nsteps, c.frame_len, c.depth);
        HIPCHECK(h2d_small(bufs[S.car_buf].d, S.carriers.data(), S.carriers.size() * sizeof(DCarrier)));
        {
            const RsCtl ctl = make_ctl(S);
            HIPCHECK(h2d_small(bufs[S.ctl_buf].d, &ctl, sizeof(RsCtl)));
        }
    }
    if (dbg_t)
        std::fprintf(stderr, "[sigops] finalize: leaves and carriers patched, carrier blocks uploaded: %.3f ms\n",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count());
    upload_tables(this);
    if (dbg_t)
        std::fprintf(stderr, "[sigops] finalize: tables uploaded: %.3f ms\n",
                     std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - tf0).count());
    // step list: stages in increasing node order (children first), then the root program
    std::vector<int> order;
    for (size_t i = 0; i < stages.size(); ++i)
        if (stages[i].need > 0) order.push_back((int)i);
    std::sort(order.begin(), order.end(), [&](int a, int b) { return stages[a].node < stages[b].node; });
    std::vector<char> batch_pushed(batches.size(), 0);
    std::vector<char> rsb_pushed(rsbatches.size(), 0);
    for (int sid : order) {
        Stage& S = stages[sid];
        if (S.batch >= 0) {  // one step for the whole batch, where its first member stood (members wait for nothing)
            if (batch_pushed[S.batch]) continue;
            batch_pushed[S.batch] = 1;
            Step st{2, S.batch, "k_sos_batch", 0};
            for (int m : batches[S.batch].members)
                st.bytes += 2 * (stages[m].need - stages[m].base) * stages[m].sg.nch * (int64_t)dsize(nodes[stages[m].node].dtype);
            steps.push_back(st);
            continue;
        }
        if (S.rsb >= 0) {  // ... and one for the plain filters that go through k_rsos together
            if (rsb_pushed[S.rsb]) continue;
            rsb_pushed[S.rsb] = 1;
            Step st{3, S.rsb, "k_rsos_batch", 0};
            for (int m : rsbatches[S.rsb].members) {
                const Stage& M = stages[m];
                const int64_t esz = (int64_t)dsize(nodes[M.node].dtype);
                st.bytes += (M.rs.n_in * (int64_t)dsize(M.carriers[0].dtype) + M.rs.n_out * esz) * M.rs.nch;
            }
            steps.push_back(st);
            continue;
        }
        if (S.pw_step >= 0) push_pw_step(S.pw_step);
        for (auto& sd : S.side)
            if (sd.pw_step >= 0) push_pw_step(sd.pw_step);
        if (S.fused_away) continue;  // (runs inside its consumer's launch)
        Step st{1, sid, stage_step_name(S), 0};
        st.bytes = stage_step_bytes(this, sid);
        steps.push_back(st);
    }
    stats.n_stages = (int)order.size() + 1;
    stats.algorithmic_bytes = algo_bytes + out.nframes * (int64_t)out.nch * (int64_t)dsize(out.dtype);
    int64_t h2d = 0;
    for (auto& h : host_leaves) h2d += (int64_t)h.bytes;
    stats.h2d_bytes = h2d;
    stats.d2h_bytes = out.is_device ? 0 : out.nframes * (int64_t)out.nch * (int64_t)dsize(out.dtype);
}

// Dependencies between steps from the plan buffers they read and write, then a lane (stream)
// per step: a step continues on the lane of its latest dependency, a step without
// dependencies opens the next lane (round robin over at most 8).
void Plan::plan_lanes() {
    const int n = (int)steps.size();
    step_deps.assign(n, {});
    step_lane.assign(n, 0);
    step_signals.assign(n, 0);
    nlanes = 1;
    if (n < 3 || std::getenv("SIGOPS_SINGLE_STREAM")) return;
    const int kFinal = -2;
    std::vector<std::set<int>> rd(n), wr(n);
    auto piece_reads = [&](const PwStep& w, std::set<int>& out) {
        for (int li : w.rtc_leaves)  // (a hipRTC step has no programs: its source names these leaves)
            if (li >= 0 && li < (int)leaves.size() && leaves[li].buf >= 0) out.insert(leaves[li].buf);
        for (int pi = w.piece0; pi < w.piece0 + w.npieces; ++pi) {
            const DPiece& P = pieces[pi];
            for (int k = 0; k < P.frame_len + P.samp_len; ++k) {
                const DOp& o = k < P.frame_len ? ops[P.frame_pc + k] : ops[P.samp_pc + (k - P.frame_len)];
                if ((o.code == OP_LOAD || o.code == OP_SCALAR) && o.arg >= 0 && o.arg < (int)leaves.size() &&
                    leaves[o.arg].buf >= 0)
                    out.insert(leaves[o.arg].buf);
            }
        }
    };
    auto carrier_reads = [&](const std::vector<DCarrier>& cs, std::set<int>& out) {
        for (auto& c : cs) {
            if (c.buf >= 0) out.insert(c.buf);
            for (int k = 0; k < c.frame_len; ++k) {
                const DOp& o = ops[c.frame_pc + k];
                if ((o.code == OP_LOAD || o.code == OP_SCALAR) && leaves[o.arg].buf >= 0) out.insert(leaves[o.arg].buf);
            }
            for (int k = 0; k < c.nslots; ++k)
                if (leaves[c.slot_leaf[k]].buf >= 0) out.insert(leaves[c.slot_leaf[k]].buf);
        }
    };
    for (int i = 0; i < n; ++i) {
        const Step& st = steps[i];
        if (st.kind == 0) {
            const PwStep& w = pw[st.idx];
            piece_reads(w, rd[i]);
            wr[i].insert(w.out_buf >= 0 ? w.out_buf : kFinal);
            // the root launch runs in place on the windows stages have written, and so does any
            // sub-expression of it that was materialised into a temporary first
            if (w.out_buf < 0 || (out_alias_buf >= 0 && rd[i].count(out_alias_buf)))
                for (size_t k = 0; k < stages.size(); ++k)
                    if (stages[k].win_off >= 0) rd[i].insert(-100 - (int)k);
        } else if (st.kind == 2) {  // members read device arrays only; each writes its window or buffer
            for (int m : batches[st.idx].members) {
                const Stage& S = stages[m];
                if (S.win_off >= 0) wr[i].insert(-100 - m);
                else wr[i].insert(m == alias_stage ? kFinal : S.out_buf);
            }
        } else if (st.kind == 3) {  // every member reads through its carriers and writes its window or buffer
            for (int m : rsbatches[st.idx].members) {
                const Stage& S = stages[m];
                carrier_reads(S.carriers, rd[i]);
                if (S.win_off >= 0) wr[i].insert(-100 - m);
                else wr[i].insert(m == alias_stage ? kFinal : S.out_buf);
            }
        } else {
            const Stage& S = stages[st.idx];
            if (S.in_buf >= 0 && S.rsos_src < 0) rd[i].insert(S.in_buf);
            for (auto& sd : S.side)
                if (sd.buf >= 0) rd[i].insert(sd.buf);
            carrier_reads(S.rsos_src >= 0 ? stages[S.rsos_src].carriers : S.carriers, rd[i]);
            if (S.win_off >= 0) wr[i].insert(-100 - st.idx);  // its own window of the result
            else wr[i].insert(st.idx == alias_stage ? kFinal : S.out_buf);
            if (S.kind == ST_NORM) {  // reads its own output buffer, writes the rms scalar
                rd[i].insert(S.out_buf);
                if (S.rms_buf >= 0) wr[i].insert(S.rms_buf);
            }
        }
    }
    auto meets = [](const std::set<int>& a, const std::set<int>& b) {
        for (int x : a)
            if (b.count(x)) return true;
        return false;
    };
    for (int i = 0; i < n; ++i)
        for (int j = 0; j < i; ++j)
            if (meets(rd[i], wr[j]) || meets(wr[i], wr[j]) || meets(wr[i], rd[j])) step_deps[i].push_back(j);
    int next = 0;
    const int kMaxLanes = 8;
    for (int i = 0; i < n; ++i) {
        if (step_deps[i].empty()) {
            step_lane[i] = next % kMaxLanes;
            ++next;
        } else step_lane[i] = step_lane[step_deps[i].back()];
    }
    step_lane[n - 1] = 0;  // the last step (it produces the result) runs on the caller's stream
    for (int i = 0; i < n; ++i) nlanes = std::max(nlanes, step_lane[i] + 1);
    for (int i = 0; i < n; ++i)
        for (int j : step_deps[i])
            if (step_lane[j] != step_lane[i]) step_signals[j] = 1;
    if (nlanes == 1) return;
    lane_streams.assign(nlanes, nullptr);
    for (int l = 1; l < nlanes; ++l) HIPCHECK(hipStreamCreateWithFlags(&lane_streams[l], hipStreamNonBlocking));
    step_done.assign(n, nullptr);
    for (int i = 0; i < n; ++i) HIPCHECK(hipEventCreateWithFlags(&step_done[i], hipEventDisableTiming));
    HIPCHECK(hipEventCreateWithFlags(&ev_start, hipEventDisableTiming));
}

void Plan::release() {
    for (auto st_ : lane_streams)
        if (st_) (void)hipStreamDestroy(st_);
    lane_streams.clear();
    for (auto e : step_done)
        if (e) (void)hipEventDestroy(e);
    step_done.clear();
    if (ev_start) (void)hipEventDestroy(ev_start);
    ev_start = nullptr;
    if (graph_exec) (void)hipGraphExecDestroy(graph_exec);
    graph_exec = nullptr;
    if (capture_stream) (void)hipStreamDestroy(capture_stream);
    capture_stream = nullptr;
    for (auto& b : bufs)
        if (b.d && !b.external) (void)hipFree(b.d);
    bufs.clear();
    if (d_pieces) (void)hipFree(d_pieces);
    if (d_ops) (void)hipFree(d_ops);
    if (d_leaves) (void)hipFree(d_leaves);
    if (kerr) {
        // (the hipFree calls above synchronised the device: whatever the plan's last launch had to say is in the word now.  An
        //  execute into a device result returns before its kernels have run, and the caller may never make another call on
        //  this plan -- a one-shot sink: so_plan_check is the call that reports it; where the host destroys the plan without
        //  it, the result it holds is invalid and nobody has been told: say so as loudly as a library can)
        (void)hipDeviceSynchronize();
        const uint32_t who = *(volatile uint32_t*)kerr;
        if (who)
            std::fprintf(stderr, "libsigops: %s: a wait between its waves did not end -- THE LAST RESULT OF THIS PLAN IS INVALID (so_plan_destroy "
                                 "without so_plan_check)\n", who == 2 ? "k_resample_arb" : "k_rsos");
        (void)hipHostFree(kerr);
    }
    kerr = nullptr;
    for (auto e : events) (void)hipEventDestroy(e);
    events.clear();
}


// executes a deferred-profiling plan keeps events for (plans of hundreds of steps keep fewer)
static size_t prof_cap(const Plan* P) {
    const size_t evset = 2 * std::max<size_t>(1, P->steps.size());
    return std::max<size_t>(1, std::min<size_t>(kProfExecs, 8192 / evset));
}

// the plan's host-mapped word a kernel reports a wait between its waves in that did not end (device address, or null: the
// kernel then traps -- also the choice of SIGOPS_RSOS_TRAP=1)
static uint32_t* kernel_error_word(Plan* P) {
    if (std::getenv("SIGOPS_RSOS_TRAP")) return nullptr;
    if (!P->kerr) {
        if (hipHostMalloc((void**)&P->kerr, 64, hipHostMallocMapped) == hipSuccess) *P->kerr = 0;
        else {
            P->kerr = nullptr;
            (void)hipGetLastError();
            return nullptr;
        }
    }
    void* dp = nullptr;
    if (hipHostGetDevicePointer(&dp, P->kerr, 0) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
    }
    return (uint32_t*)dp;
}

// a kernel gave up on a wait between its waves (k_rsos: a protocol that did not hold; its result and
// everything computed from it is wrong): reported once: by the execute itself where it synchronises (a host result), else by the next call on the plan
static bool kernel_gave_up(Plan* P, std::string& err) {
    if (!P->kerr || !*(volatile uint32_t*)P->kerr) return false;
    const uint32_t who = *(volatile uint32_t*)P->kerr;  // 1: k_rsos, 2: k_resample_arb
    *(volatile uint32_t*)P->kerr = 0;
    err = std::string(who == 2 ? "k_resample_arb" : "k_rsos") + ": a wait between its waves did not end (this plan's last result is invalid)";
    return true;
}

// ---------------------------------------------------------------------------
// Where a stage reads and writes: the first element and the channel pitch in elements.
struct View {
    char* d;
    int64_t pitch;
};
static const char* array_base(Plan* P, int an) {
    return P->nodes[an].nd.i0 ? (const char*)P->array_ptr[an] : (const char*)P->bufs[P->array_buf[an]].d;
}
// The input Plan::stage_input set up: a caller's array where it lies, or a plan buffer, whose first element is the node's
// frame `frame0`.  `dtype` is the type of the samples where they lie: the child's for SampleAt, Comb and Cumsum, the node's
// own for the filters and resamplers.  A stage with neither (a filter whose source k_rsos reads through carriers) has no view.
static View stage_in(Plan* P, const Stage& S, int nch, int dtype) {
    if (S.in_array_node >= 0)
        return View{(char*)array_base(P, S.in_array_node) + (size_t)S.in_offset * dsize(dtype), nch == 1 ? 0 : S.in_pitch};
    if (S.in_buf < 0) return View{nullptr, 0};
    const Buf& b = P->bufs[S.in_buf];
    return View{(char*)b.d + (size_t)(S.in_offset - b.frame0) * dsize(dtype), b.pitch};
}
// Where stage `sid` writes: its own buffer; the sink's result where the stage is aliased to it (Plan::alias_stage), from
// the stage's local frame alias_skip on -- earlier frames are not stored, and the skipped frames are counted in the type
// the stage stores, the result's where it rounds to it (alias_narrow); or its window of the result (Stage::win_off), which
// has the node's type (try_window_alias takes stages of the result's type only).
// SampleAt, Comb and Cumsum, whose kernels store Float64 only, get 8 bytes for both: their nodes are Float64 (build_nodes),
// and plan_create lets only a periodic resampler or a filter narrow, so alias_narrow is false where one of them is aliased.
// Moving stores its node's type, Float32 or Float64, and is aliased only to a result of that type.
// Movsum, Recur and Recur2 store Float64 like Cumsum: their nodes are Float64.
// A member of an RsBatch is never the aliased stage (fuse_plain_sos skips it): k_rsos_batch's members write windows or buffers.
static View stage_out(Plan* P, int sid, void* outp) {
    const Stage& S = P->stages[sid];
    const Node& N = P->nodes[S.node];
    const size_t esz = dsize(N.dtype);
    if (sid == P->alias_stage) {
        View v{(char*)outp, N.nch == 1 ? std::max<int64_t>(P->out.chan_stride, S.need) : P->out.chan_stride};
        if (!P->out.is_device) v = View{(char*)P->bufs[P->out_stage_buf].d, P->bufs[P->out_stage_buf].pitch};  // (a host result: its staging buffer)
        v.d -= (size_t)P->alias_skip * (P->alias_narrow ? dsize(P->out.dtype) : esz);
        return v;
    }
    if (S.win_off >= 0) {
        const Buf& ab = P->bufs[P->out_alias_buf];
        return View{(char*)(P->out.is_device ? outp : ab.d) + (size_t)S.win_off * esz, ab.pitch};
    }
    const Buf& ob = P->bufs[S.out_buf];
    return View{(char*)ob.d, ob.pitch};
}

// the fused sine source of a cascade's input (Stage::src_op): the generator's leaf and one step of its rotation
static void set_sine_source(SosGeom& g, const Stage& S) {
    const DLeaf& F = S.src_fn;
    g.src_op = S.src_op;
    g.src_has_omega = F.flag;
    g.src_df = F.df;
    g.src_omega = F.v0;
    g.src_phi = F.v1;
    g.src_fs = F.v2;
    const double step = 6.283185307179586476925 * (F.flag ? F.v0 / F.v2 : 1.0 / F.v2);
    g.src_cd = std::cos(step);
    g.src_sd = std::sin(step);
}
// what a kernel that reads through stage S's carriers reads them with
static RsGlobalTables global_tables(Plan* P, const Stage& S) {
    return RsGlobalTables{(const RsCtl*)P->bufs[S.ctl_buf].d, (const DCarrier*)P->bufs[S.car_buf].d, P->d_ops, P->d_leaves};
}
// what k_rsos_fixup needs behind a k_rsos launch of filter S: what that launch was given (I), the reference's taps, the sections
static void set_rsos_fixup(RsFixup& F, Plan* P, const Stage& S, const RsosItem& I) {
    F.g = I.g;
    F.tab = I.tab;
    F.jend = I.jend;
    F.jrel = (const int*)P->bufs[S.rsos_jrel_buf].d;
    F.taps = S.rsos_taps;
    F.cf = S.groups[0];
    F.gsrc = I.gsrc;
    F.y = I.y;
}
// "no non-finite chunk (range) yet" in every word of a SosGeom::bad / RsSos::bad array
static void arm_bad(void* words, size_t n, hipStream_t st) { HIPCHECK((hipError_t)launch_fill_u32(words, n, 0x7f7f7f7fu, st)); }
// after an execute that failed nobody knows what its launches left in the words: the next one arms them itself (run_rsos_fused)
static void disarm_bad(Plan* P) {
    for (const Stage& S : P->stages) S.bad_armed = false;
}

// The tuning aids' traces: the cycle stamps workgroup 0 of a launch left (waits for it), printed relative to the earliest, t0.
static std::vector<long long> read_trace(const long long* d_trace, size_t trace_n, hipStream_t st, long long& t0) {
    std::vector<long long> tr(trace_n);
    HIPCHECK(hipStreamSynchronize(st));
    HIPCHECK(hipMemcpy(tr.data(), d_trace, trace_n * 8, hipMemcpyDeviceToHost));
    t0 = 0;
    for (size_t i = 0; i < trace_n; ++i)
        if (tr[i] && (!t0 || tr[i] < t0)) t0 = tr[i];
    return tr;
}
// SIGOPS_RS_TRACE: k_resample_periodic's
static void dump_rs_trace(const long long* d_trace, size_t trace_n, const RsPeriodic& rp, hipStream_t st) {
    long long t0;
    const std::vector<long long> tr = read_trace(d_trace, trace_n, st, t0);
    for (int w = 0; w < rp.nwaves; ++w)
        for (int it = 0; it < kRsTraceIters; ++it) {
            const long long* q = &tr[((size_t)w * kRsTraceIters + it) * kRsTraceStamps];
            if (!q[0]) continue;
            std::fprintf(stderr, "[rs-trace] %s w%02d it%02d", w < rp.ncompute ? "C" : "L", w, it);
            for (int k = 0; k < kRsTraceStamps; ++k) std::fprintf(stderr, " %lld", q[k] ? q[k] - t0 : -1);
            std::fprintf(stderr, "\n");
        }
}
// SIGOPS_RSOS_TRACE: k_rsos's; =2 (a -DSO_RSOS_COUNT=1 build): its poll counters, raw
static void dump_rsos_trace(const long long* d_trace, size_t trace_n, const RsSos& rs, hipStream_t st) {
    long long t0;
    const std::vector<long long> tr = read_trace(d_trace, trace_n, st, t0);
    const bool counters = std::atoi(std::getenv("SIGOPS_RSOS_TRACE")) == 2;
    for (int w = 0; w < rs.nwaves; ++w)
        for (int it = 0; it < (counters ? 5 : kRsosTraceIters); ++it) {
            const long long* q = &tr[((size_t)w * kRsosTraceIters + it) * 8];
            if (counters) {
                bool any = false;
                for (int k = 0; k < 8; ++k) any = any || q[k];
                if (!any) continue;
                std::fprintf(stderr, "[rsos-count] w%02d row%d", w, it);
                for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %lld", q[k] - 1);
            } else {
                if (!q[0] && !q[2]) continue;
                std::fprintf(stderr, "[rsos-trace] %s w%02d it%02d", w == 0 ? "C" : (w & 3) == 0 ? "L" : "Y", w, it);
                for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %lld", q[k] ? q[k] - t0 : -1);
            }
            std::fprintf(stderr, "\n");
        }
    for (int w = 0; w < rs.nwaves && w < 16 && !counters; ++w) {  // the prologue of the first group (rsos_stamp_pro's columns)
        const long long* q = &tr[((size_t)16 * kRsosTraceIters + w) * 8];
        std::fprintf(stderr, "[rsos-trace-pro] w%02d", w);
        for (int k = 0; k < 8; ++k) std::fprintf(stderr, " %lld", q[k] ? q[k] - t0 : -1);
        std::fprintf(stderr, "\n");
    }
}

// ---------------------------------------------------------------------------
// One routine per kind of step.  Each issues the step's launches on `st` and returns how many it issued (Step::launches).

static int run_pointwise(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const PwStep& w = P->pw[s.idx];
    if (w.nblocks <= 0) return 0;  // empty rectangle (zero-frame sink): nothing to launch
    static const int il_scalar = std::getenv("SIGOPS_K1_ILSCALAR") ? 1 : 0;  // ablation knob
    OutView ov{};  // a plan buffer, the device result with its own strides, or a host result's staging buffer
    if (w.out_buf >= 0) {
        const Buf& b = P->bufs[w.out_buf];
        ov = OutView{b.d, 1, b.pitch, b.dtype, il_scalar};
    } else if (P->out.is_device) {
        ov = OutView{outp, P->out.frame_stride, P->out.chan_stride, P->out.dtype, il_scalar};
    } else {
        const Buf& b = P->bufs[P->out_stage_buf];
        ov = OutView{b.d, P->interleaved_host ? P->out.nch : 1, P->interleaved_host ? 1 : b.pitch, b.dtype, il_scalar};
    }
    if (w.fill)
        launch_randn_fill(P->d_pieces + w.piece0, w.npieces, w.nblocks, P->d_leaves, ov, st);
    else if (w.rtc) {
        if (rtc_launch(w.rtc, w.nblocks, P->d_pieces + w.piece0, w.npieces, P->d_leaves, ov, st) != 0)
            fail(SO_ERR_RUNTIME, "hipRTC kernel launch failed");
    } else
        launch_pointwise(P->d_pieces + w.piece0, w.npieces, w.nblocks, P->d_ops, P->d_leaves, ov, w.deep, st, w.chain,
                         w.il || (ov.fstride > 1 && ov.cstride == 1), w.math);
    return 1;
}

// independent filters of one shape, their three passes in three launches (k_sos_batch): a descriptor per member
static int run_sos_batch(Plan* P, const Step& s, void* outp, hipStream_t st) {
    SosBatch& B = P->batches[s.idx];
    const size_t nm = B.members.size();
    const bool poison = B.bad_buf >= 0 && !std::getenv("SIGOPS_SOS_NOPOISON");
    std::vector<SosDesc> d(nm + 1);
    int64_t first[3] = {0, 0, 0};
    for (size_t m = 0; m <= nm; ++m) {
        SosDesc& D = d[m];
        std::memset(&D, 0, sizeof D);
        for (int q = 0; q < 3; ++q) D.first[q] = first[q];
        if (m == nm) break;
        const int sid = B.members[m];
        const Stage& S = P->stages[sid];
        const Node& N = P->nodes[S.node];
        const View in = stage_in(P, S, N.nch, N.dtype), out = stage_out(P, sid, outp);
        D.x = in.d;
        D.y = out.d;
        D.v = S.v_buf >= 0 ? (double*)P->bufs[S.v_buf].d : nullptr;
        D.s0 = S.s0_buf >= 0 ? (double*)P->bufs[S.s0_buf].d : nullptr;
        D.mpow = S.mpow_buf >= 0 ? (const double*)P->bufs[S.mpow_buf].d : nullptr;
        D.g = S.sg;
        D.g.in_pitch = in.pitch;
        D.g.out_pitch = out.pitch;
        D.g.store_lo = sid == P->alias_stage ? P->alias_skip : 0;
        if (sid == P->alias_stage && P->alias_narrow) D.g.out_dtype = SO_F32;
        D.g.align_rows = !std::getenv("SIGOPS_SOS_NOALIGN");
        D.g.bad = poison && S.sg.nchunks > 1 ? (int32_t*)P->bufs[B.bad_buf].d + B.bad_off[m] : nullptr;
        if (S.src_op) set_sine_source(D.g, S);
        D.cf = S.groups[0];
        const int64_t nseq = (int64_t)D.g.nchunks * D.g.nch;
        if (D.g.nchunks > 1) {
            first[0] += ((int64_t)(D.g.nchunks - 1) * D.g.nch + kBlock - 1) / kBlock;
            first[1] += (nseq + kBlock - 1) / kBlock;
        } else
            D.s0 = nullptr;  // one chunk: starts from rest
        first[2] += (nseq + kBlock - 1) / kBlock;
    }
    if (first[2] >= ((int64_t)1 << 31)) fail(SO_ERR_RUNTIME, "internal: batched IIR grid too large");
    if (B.host.size() != d.size() || std::memcmp(B.host.data(), d.data(), d.size() * sizeof(SosDesc)) != 0) {
        // the descriptors change only when the result or an array moves -- never between the direct execute for a result
        // pointer and the capture that follows it (plan_execute), so a captured graph holds the three launches only and
        // reads the table this copy left on the device
        B.host = d;
        HIPCHECK(hipMemcpyAsync(P->bufs[B.desc_buf].d, B.host.data(), B.host.size() * sizeof(SosDesc), hipMemcpyHostToDevice, st));
    }
    for (int q = 0; q < 3; ++q) B.total[q] = first[q];
    if (poison) arm_bad(P->bufs[B.bad_buf].d, P->bufs[B.bad_buf].bytes / 4, st);
    int nl = launch_sos_batch((const SosDesc*)P->bufs[B.desc_buf].d, (int)nm, B.nsec, B.dtype, B.total, st);
    if (poison) nl += launch_sos_poison_batch((const SosDesc*)P->bufs[B.desc_buf].d, (int)nm, B.dtype, st);
    return nl;
}

// plain filters, one pass each, ONE launch (k_rsos_batch): per member what run_rsos_fused sets up for a launch of its own
static int run_rsos_batch(Plan* P, const Step& s, void* outp, hipStream_t st) {
    RsBatch& B = P->rsbatches[s.idx];
    const size_t nm = B.members.size();
    std::vector<RsosItem> items(nm);
    std::vector<RsFixup> fix(nm);
    const bool poison = B.bad_buf >= 0 && !std::getenv("SIGOPS_SOS_NOPOISON");
    int maxch = 1, out_f32 = 0;
    for (size_t m = 0; m < nm; ++m) {
        const int sid = B.members[m];
        const Stage& S = P->stages[sid];
        const View out = stage_out(P, sid, outp);
        RsosItem& I = items[m];
        std::memset(&I, 0, sizeof I);
        RsSos rs = S.rs;
        rs.out_pitch = out.pitch;
        rs.out_f32 = P->nodes[S.node].dtype == SO_F32;
        rs.f32m = 0;
        rs.sring = 0;
        rs.mats = (const double*)P->bufs[S.rsos_mats_buf].d;
        rs.bad = poison ? (int32_t*)P->bufs[B.bad_buf].d + B.bad_off[m] : nullptr;
        rs.err = kernel_error_word(P);
        I.g = rs;
        I.tab = (const double*)P->bufs[S.rsos_tab_buf].d;
        I.jend = (const int*)P->bufs[S.rsos_jend_buf].d;
        I.y = out.d - (size_t)S.rs.store_lo * (rs.out_f32 ? 4 : 8);
        I.gsrc = global_tables(P, S);
        std::memset(&fix[m], 0, sizeof fix[m]);
        set_rsos_fixup(fix[m], P, S, I);
        maxch = std::max(maxch, (int)rs.nch);
        out_f32 = rs.out_f32;
    }
    if (B.host.size() != nm || std::memcmp(B.host.data(), items.data(), nm * sizeof(RsosItem)) != 0 ||
        std::memcmp(B.fhost.data(), fix.data(), nm * sizeof(RsFixup)) != 0) {
        // (as the three-pass batch's descriptors: the tables change only when the result or an array moves -- never
        //  between the direct execute for a result pointer and the capture that follows it)
        B.host = items;
        B.fhost = fix;
        HIPCHECK(hipMemcpyAsync(P->bufs[B.items_buf].d, B.host.data(), nm * sizeof(RsosItem), hipMemcpyHostToDevice, st));
        HIPCHECK(hipMemcpyAsync(P->bufs[B.fix_buf].d, B.fhost.data(), nm * sizeof(RsFixup), hipMemcpyHostToDevice, st));
    }
    if (poison) arm_bad(P->bufs[B.bad_buf].d, P->bufs[B.bad_buf].bytes / 4, st);
    if (launch_rsos_batch((const RsosItem*)P->bufs[B.items_buf].d, (int)nm, B.gpm, items[0].g, st) != 0)
        fail(SO_ERR_RUNTIME, "internal: no batched one-pass IIR instantiation for this geometry");
    int nl = 1;
    if (poison) nl += launch_rsos_fixup_batch((const RsFixup*)P->bufs[B.fix_buf].d, (int)nm, maxch, out_f32, st);
    return nl;
}

static int run_sample_at(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const int xdt = P->nodes[N.kids[0]].dtype;
    const View in = stage_in(P, S, N.nch, xdt), out = stage_out(P, s.idx, outp);
    SampleAtArgs a{};
    a.x = in.d;
    a.xcs = in.pitch;
    a.xfs = S.x_fstride;
    a.N = S.in_frames;
    a.x_f32 = xdt == SO_F32;
    if (S.side[0].array_node >= 0) {
        a.pos = (const double*)array_base(P, S.side[0].array_node) + S.side[0].offset;
        a.pcs = S.side[0].pitch;
    } else {
        const Buf& b = P->bufs[S.side[0].buf];
        a.pos = (const double*)b.d;
        a.pcs = S.side[0].pitch == 0 ? 0 : b.pitch;
    }
    a.y = (double*)out.d;
    a.ycs = out.pitch;
    a.base = S.base;
    a.n = S.need - S.base;
    a.left = N.nd.d0;
    a.right = N.nd.d1;
    a.nch = N.nch;
    a.relative = N.nd.i0 & 1;
    a.wrap = (N.nd.i0 >> 1) & 1;
    int nl;
    if (N.nd.i1 == 0) {
        nl = launch_sample_at(a, st);
    } else {
        SampleAtFirArgs f{};
        f.a = a;
        f.kind = N.nd.i1;
        f.K = N.nd.i1 == 2 ? N.nd.i2 : 4;
        f.tab = S.sa_tab_buf >= 0 ? (const double*)P->bufs[S.sa_tab_buf].d : nullptr;
        nl = launch_sample_at_fir(f, st);
    }
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "SampleAt: more than 65535 channels or 2^39 frames are not lowered");
    return nl;
}

static int run_comb(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const int xdt = P->nodes[N.kids[0]].dtype;
    const View in = stage_in(P, S, N.nch, xdt), out = stage_out(P, s.idx, outp);
    CombArgs a{};
    a.x = in.d;
    a.xcs = in.pitch;
    a.xfs = S.x_fstride;
    a.x_f32 = xdt == SO_F32;
    a.y = (double*)out.d;
    a.ycs = out.pitch;
    a.n = S.need - S.base;  // (a carried state: the rows start at the resume frame, Plan::process_from_frame_0)
    a.r = S.base;
    a.cin = (const double*)N.nd.p0;
    a.cout = (double*)const_cast<void*>(N.nd.p1);
    a.D = N.nd.l0;
    a.b0 = N.nd.d0;
    a.bD = N.nd.d1;
    a.a = N.nd.d2;
    a.nch = N.nch;
    if (a.D < 1) fail(SO_ERR_INVALID, "Comb: a delay of less than one frame");  // (the planner has refused it)
    const int nl = launch_comb(a, st);
    // (one lane per frame mod D: min(D, frames) lanes a channel, in blocks of kBlock, must fit grid.x)
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "Comb: more than 65535 channels, or a delay AND a signal of 2^39 frames and more, are not lowered");
    return nl;
}

static int run_cumsum(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const int xdt = P->nodes[N.kids[0]].dtype;
    const View in = stage_in(P, S, N.nch, xdt), out = stage_out(P, s.idx, outp);
    CumsumArgs a{};
    a.x = in.d;
    a.xcs = in.pitch;
    a.xfs = S.x_fstride;
    a.x_f32 = xdt == SO_F32;
    a.y = (double*)out.d;
    a.ycs = out.pitch;
    a.n = S.need - S.base;  // (a carried state: the rows start at the resume frame, Plan::process_from_frame_0)
    a.k0 = S.base / kCumsumChunk;
    a.cin = (const double*)N.nd.p0;
    a.cout = (double*)const_cast<void*>(N.nd.p1);
    a.nch = N.nch;
    a.tot_pitch = cumsum_totals(a.n);
    a.tot = S.aux_buf >= 0 ? (double*)P->bufs[S.aux_buf].d : nullptr;
    const int nl = launch_cumsum(a, st);
    // (one workgroup per chunk of kCumsumChunk frames in grid.x, the channels in grid.y)
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "Cumsum: more than 65535 channels, or 2^31 chunks of 16384 frames and more, are not lowered");
    return nl;
}

static int run_recur(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const bool row = N.kids.size() == 2;
    const int bdt = P->nodes[N.kids[row ? 1 : 0]].dtype;
    const View in = stage_in(P, S, N.nch, bdt), out = stage_out(P, s.idx, outp);
    RecurArgs a{};
    a.b = in.d;
    a.bcs = in.pitch;
    a.bfs = S.x_fstride;
    a.b_f32 = bdt == SO_F32;
    if (!row) {
        a.ac = N.nd.d0;
    } else if (S.side[0].array_node >= 0) {
        a.a = (const double*)array_base(P, S.side[0].array_node) + S.side[0].offset;
        a.acs = S.side[0].pitch;
    } else {
        const Buf& b = P->bufs[S.side[0].buf];
        a.a = (const double*)b.d;
        a.acs = S.side[0].pitch == 0 ? 0 : b.pitch;
    }
    a.y = (double*)out.d;
    a.ycs = out.pitch;
    a.n = S.need - S.base;  // (a carried state: the rows start at the resume frame, Plan::process_from_frame_0)
    a.k0 = S.base / kCumsumChunk;
    a.cin = (const double*)N.nd.p0;
    a.cout = (double*)const_cast<void*>(N.nd.p1);
    a.nch = N.nch;
    a.op = N.nd.i0;
    a.tot_pitch = cumsum_totals(a.n);
    a.tot = S.aux_buf >= 0 ? (double*)P->bufs[S.aux_buf].d : nullptr;
    const int nl = launch_recur(a, st);
    // (one workgroup per chunk of kCumsumChunk frames in grid.x, the channels in grid.y)
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "Recur: more than 65535 channels, or 2^31 chunks of 16384 frames and more, are not lowered");
    return nl;
}

static int run_recur2(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const bool row = N.kids.size() == 3;
    const int bdt = P->nodes[N.kids[row ? 2 : 0]].dtype;
    const View in = stage_in(P, S, N.nch, bdt), out = stage_out(P, s.idx, outp);
    Recur2Args a{};
    a.b = in.d;
    a.bcs = in.pitch;
    a.bfs = S.x_fstride;
    a.b_f32 = bdt == SO_F32;
    a.ac[0] = N.nd.d0, a.ac[1] = N.nd.d1;
    for (int w = 0; row && w < 2; ++w) {
        const Stage::Side& sd = S.side[w];
        if (sd.array_node >= 0) {
            a.a[w] = (const double*)array_base(P, sd.array_node) + sd.offset;
            a.acs[w] = sd.pitch;
        } else {
            const Buf& b = P->bufs[sd.buf];
            a.a[w] = (const double*)b.d;
            a.acs[w] = sd.pitch == 0 ? 0 : b.pitch;
        }
    }
    a.y = (double*)out.d;
    a.ycs = out.pitch;
    a.n = S.need - S.base;  // (a carried state: the rows start at the resume frame, Plan::process_from_frame_0)
    a.k0 = S.base / kCumsumChunk;
    a.cin = (const double*)N.nd.p0;
    a.cout = (double*)const_cast<void*>(N.nd.p1);
    a.nch = N.nch;
    a.tot_pitch = cumsum_totals(a.n);
    a.tot = S.aux_buf >= 0 ? (double*)P->bufs[S.aux_buf].d : nullptr;
    const int nl = launch_recur2(a, st);
    // (one workgroup per chunk of kCumsumChunk frames in grid.x, the channels in grid.y)
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "Recur2: more than 65535 channels, or 2^31 chunks of 16384 frames and more, are not lowered");
    return nl;
}

static int run_moving(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const View in = stage_in(P, S, N.nch, N.dtype), out = stage_out(P, s.idx, outp);
    MovingArgs a{};
    a.x = in.d;
    a.xcs = in.pitch;
    a.xfs = S.x_fstride;
    a.n_in = S.in_frames;
    a.y = out.d;
    a.ycs = out.pitch;
    a.n_out = S.need - S.base;
    a.off = S.base - S.in_base;
    a.back = N.nd.l0;
    a.ahead = N.nd.l1;
    a.tab = S.aux_buf >= 0 ? P->bufs[S.aux_buf].d : nullptr;
    a.nch = N.nch;
    a.f32 = N.dtype == SO_F32;
    a.is_min = N.nd.i0;
    const int nl = launch_moving(a, st);
    // (one workgroup per tile of kMovTile frames in grid.x, the channels in grid.y)
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "Moving: more than 65535 channels, or 2^31 tiles of 2048 frames and more, are not lowered");
    return nl;
}

static int run_movrank(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const View in = stage_in(P, S, N.nch, N.dtype), out = stage_out(P, s.idx, outp);
    MovrankArgs a{};
    a.x = in.d;
    a.xcs = in.pitch;
    a.xfs = S.x_fstride;
    a.n_in = S.in_frames;
    a.y = out.d;
    a.ycs = out.pitch;
    a.n_out = S.need - S.base;
    a.off = S.base - S.in_base;
    a.back = N.nd.l0;
    a.ahead = N.nd.l1;
    a.q = N.nd.d0;
    a.nch = N.nch;
    a.f32 = N.dtype == SO_F32;
    const int nl = launch_movrank(a, st);
    // (one workgroup per tile of kRankTile frames in grid.x, the channels in grid.y; process_moving refused a longer window)
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "Movrank: more than 65535 channels, 2^31 tiles of 2048 frames and more, or a window of more than 1025 frames, are not lowered");
    return nl;
}

static int run_movsum(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const int xdt = P->nodes[N.kids[0]].dtype;
    const View in = stage_in(P, S, N.nch, xdt), out = stage_out(P, s.idx, outp);
    MovsumArgs a{};
    a.x = in.d;
    a.xcs = in.pitch;
    a.xfs = S.x_fstride;
    a.x_f32 = xdt == SO_F32;
    a.n_in = S.in_frames;
    a.y = (double*)out.d;
    a.ycs = out.pitch;
    a.n_out = S.need - S.base;
    a.off = S.base - S.in_base;
    a.abs0 = S.in_base;  // the summation tree is fixed by x's own frame numbers
    a.back = N.nd.l0;
    a.ahead = N.nd.l1;
    a.tab = S.aux_buf >= 0 ? (double*)P->bufs[S.aux_buf].d : nullptr;
    a.nch = N.nch;
    a.op = N.nd.i0;
    const int nl = launch_movsum(a, st);
    // (one workgroup per tile of kMsumTile frames in grid.x, the channels in grid.y)
    if (nl < 0) fail(SO_ERR_UNSUPPORTED, "Movsum: more than 65535 channels, or 2^31 tiles of 2048 frames or blocks of 1024 frames and more, are not lowered");
    return nl;
}

// the resampler in front and this cascade in one launch (k_rsos); `g`: the cascade's geometry as run_sos set it up
static int run_rsos_fused(Plan* P, const Stage& S, const SosGeom& g, const View& out, hipStream_t st) {
    const Node& N = P->nodes[S.node];
    const Stage& S3 = P->stages[S.rsos_src];
    RsSos rs = S.rs;
    rs.out_pitch = out.pitch;
    rs.out_f32 = g.out_dtype == SO_F32 || N.dtype == SO_F32;
    if (rs.f32m && rs.out_f32) rs.ring32 = 1;  // (a Float32 result: Float32 samples in the ring, the Float32 MFMA)
    else rs.f32m = 0;
    rs.sring = rs.f32m && (rs.fuse == 1 || rs.fuse == 2) && !std::getenv("SIGOPS_RSOS_NO_SRING") ? 1 : 0;
    // the kernel's output m is frame m - store_lo of this stage's buffer (a window: the resampler's warm
    // start lies store_lo frames before the cascade's); the sink's own skipped frames come on top
    char* const yk = out.d - (size_t)S.rs.store_lo * (rs.out_f32 ? 4 : 8);
    rs.store_lo = S.rs.store_lo + g.store_lo;
    rs.mats = (const double*)P->bufs[S.rsos_mats_buf].d;
    rs.bad = nullptr;
    const bool fixup = S.rsos_jrel_buf >= 0 && !std::getenv("SIGOPS_RSOS_NO_FIXUP");
    int rearm = 0;
    if (S.bad_buf >= 0 && rs.nranges >= 1 && !std::getenv("SIGOPS_SOS_NOPOISON")) {
        // Two sets of words.  Direct launches alternate between them: k_rsos_fixup, which every execute ends with, leaves
        // the other set armed (k_exact.hip), and the fill launch runs only where nobody has done that -- the plan's first
        // execute, and the one after an execute that failed (disarm_bad).  A captured graph holds fixed arguments and
        // k_sos_poison arms nothing: those executes use set 0 behind a fill of their own, as before.
        int32_t* const words = (int32_t*)P->bufs[S.bad_buf].d;
        const size_t nch = (size_t)N.nch;
        if (fixup && !P->graph_plan && rs.nch == N.nch && P->bufs[S.bad_buf].bytes >= 2 * nch * 4) {
            if (!S.bad_armed) {
                arm_bad(words, 2 * nch, st);
                S.bad_set = 0;
            }
            rs.bad = words + (S.bad_set ? nch : 0);
            rearm = S.bad_set ? -(int)nch : (int)nch;
        } else {
            S.bad_armed = false;
            rs.bad = words;
            arm_bad(rs.bad, nch, st);
        }
    }
    rs.err = kernel_error_word(P);
    static long long* d_rtrace = nullptr;  // SIGOPS_RSOS_TRACE tuning aid
    // (SIGOPS_RSOS_TRACE_SKIP=n: not the first n launches of the process -- a traced launch synchronises, and a run
    //  of traced launches never leaves the chip's power-management transient)
    static int rtrace_seen = 0;
    const char* const rtrace_skip = std::getenv("SIGOPS_RSOS_TRACE_SKIP");
    const bool rtracing = std::getenv("SIGOPS_RSOS_TRACE") != nullptr && rtrace_seen++ >= (rtrace_skip ? std::atoi(rtrace_skip) : 0);
    const size_t rtrace_n = (size_t)(16 * kRsosTraceIters + 16) * 8;  // (+ the prologue's rows: k_rsos.hip rsos_stamp_pro)
    if (rtracing) {
        if (!d_rtrace) HIPCHECK(hipMalloc(&d_rtrace, rtrace_n * 8));
        HIPCHECK(hipMemsetAsync(d_rtrace, 0, rtrace_n * 8, st));
        rs.trace = d_rtrace;
    }
    const double* rtab = (const double*)P->bufs[S.rsos_tab_buf >= 0 ? S.rsos_tab_buf : S3.tab_buf].d;
    const int* rjend = (const int*)P->bufs[S.rsos_jend_buf >= 0 ? S.rsos_jend_buf : S3.jend_buf].d;
    // (a folded plan's kernel reads M_g = T . Tap_g^T, behind E and C in `mats`, as its tap table; the fix-up launch recomputes single
    //  outputs the reference's way, from the taps themselves.  A Float32 result has no folded instantiation)
    if (rs.out_f32) rs.fold = 0;
    if (launch_rsos(rs.fold ? rs.mats + rs.fold_off + 7 * 64 : rtab, rjend, rs, yk, global_tables(P, S3), S.rsos_grid, st) != 0)
        fail(SO_ERR_RUNTIME, "internal: no fused resampler + IIR instantiation for this geometry");
    if (rtracing) dump_rsos_trace(d_rtrace, rtrace_n, rs, st);
    int nl = 1;
    if (rs.bad && fixup) {
        // behind a non-finite sample the reference stays non-finite: NaN over everything after the first bad
        // range -- and INSIDE that range the block the sample fell into (the block form makes all 16 outputs
        // non-finite, and a group's window is wider than an output's) output by output the reference's way
        RsFixup fx{};
        set_rsos_fixup(fx, P, S, RsosItem{rs, rtab, rjend, yk, global_tables(P, S3)});
        fx.rearm = rearm;
        nl += launch_rsos_fixup(fx, st);
        if (rearm != 0) {  // (the next execute's set, armed by this launch)
            S.bad_set ^= 1;
            S.bad_armed = true;
        }
    } else if (rs.bad) {
        SosGeom pg = g;
        pg.n = rs.n_out;
        pg.chunk = rs.pr * rs.L;
        pg.nchunks = rs.nranges;
        pg.store_lo = rs.store_lo;
        pg.bad = rs.bad;
        nl += launch_sos_poison(yk, pg, st);
    }
    return nl;
}

static int run_sos(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const size_t esz = dsize(N.dtype);
    const View in = stage_in(P, S, N.nch, N.dtype), out = stage_out(P, s.idx, outp);
    SosGeom g = S.sg;
    g.in_pitch = in.pitch;
    g.out_pitch = out.pitch;
    g.store_lo = s.idx == P->alias_stage ? P->alias_skip : 0;
    if (s.idx == P->alias_stage && P->alias_narrow) g.out_dtype = SO_F32;
    g.align_rows = S.pre_stage < 0 && !std::getenv("SIGOPS_SOS_NOALIGN");
    g.bad = nullptr;
    // (the planner fuses only what is none of the forms below: fuse_resample_sos, fuse_plain_sos)
    if (S.rsos_src >= 0) return run_rsos_fused(P, S, g, out, st);
    if (S.bad_buf >= 0 && S.pre_stage < 0 && !S.onepass && !S.xscan && !g.exact && !std::getenv("SIGOPS_SOS_NOPOISON")) {
        g.bad = (int32_t*)P->bufs[S.bad_buf].d;
        arm_bad(g.bad, (size_t)N.nch, st);
    }
    int nl = 0;
    for (size_t gi = 0; gi < S.groups.size() && S.onepass; ++gi) {
        const void* x = gi == 0 ? (const void*)in.d : (const void*)out.d;
        SosOne o = S.so1;
        o.in_pitch = gi == 0 ? in.pitch : out.pitch;
        o.out_pitch = out.pitch;
        const int64_t al = 16 / (int64_t)esz;
        o.vec_in = ((uintptr_t)x % 16 == 0) && (o.in_pitch % al == 0);
        o.vec_out = ((uintptr_t)out.d % 16 == 0) && (o.out_pitch % al == 0);
        const Buf& sb = P->bufs[S.one_sync_buf];
        const Buf& vb = P->bufs[S.one_vpub_buf];
        // (kernel nodes, not memset nodes, as for the poison words: this sequence is graph-capturable too, and a
        //  stale ticket counter would hang the kernel -- k_small.hip)
        if (sb.bytes % 4 == 0 && vb.bytes % 4 == 0) {
            HIPCHECK((hipError_t)launch_fill_u32(sb.d, sb.bytes / 4, 0u, st));           // ticket counter
            HIPCHECK((hipError_t)launch_fill_u32(vb.d, vb.bytes / 4, 0xffffffffu, st));  // "not published yet"
        } else {
            HIPCHECK(hipMemsetAsync(sb.d, 0, sb.bytes, st));
            HIPCHECK(hipMemsetAsync(vb.d, 0xff, vb.bytes, st));
        }
        launch_sos_onepass(x, out.d, o, S.groups[gi], (const double*)P->bufs[S.one_tabs_buf].d + S.one_tabs_off[gi],
                           (int*)sb.d, (double*)vb.d, N.dtype, st);
        nl += 1;
        // (behind a NaN the reference stays NaN, the look-back recovers after kt tiles: the tiles' published states tell)
        if (!std::getenv("SIGOPS_SOS_NOPOISON")) nl += launch_sos_poison_onepass(out.d, (const double*)vb.d, S.groups[gi].nsec, o, N.dtype, st);
    }
    if (S.pre_stage >= 0) {
        const Stage& S3 = P->stages[S.pre_stage];
        nl += launch_sos_prestate(in.d, out.d, (const double*)P->bufs[S3.vper_buf].d, S3.rp.nperiods,
                                  (const double*)P->bufs[S.qmat_buf].d, S3.rp.pt, (double*)P->bufs[S.v_buf].d,
                                  (double*)P->bufs[S.s0_buf].d, (const double*)P->bufs[S.mpow_buf].d, g, S.groups[0], st);
    }
    bool exact_done = false;
    if (g.exact && !S.onepass && S.pre_stage < 0 && S.groups.size() <= 2) {
        // ill-conditioned cascade: DSP.jl's order of operations, one sequence per channel
        exact_done = launch_sos_exact(in.d, out.d, g, S.groups[0], S.groups.size() > 1 ? S.groups[1] : SosCoefs{}, st) == 0;
        if (exact_done) nl += 1;
    }
    for (size_t gi = 0; gi < S.groups.size() && !S.onepass && S.pre_stage < 0 && !exact_done; ++gi) {
        // (later groups filter the output in place)
        const void* x = gi == 0 ? (const void*)in.d : (const void*)out.d;
        SosGeom gg = g;
        if (gi > 0) gg.in_pitch = out.pitch;
        if (gi == 0 && S.src_op) set_sine_source(gg, S);
        // frames beyond the child's end are zero (Pad(x.signal,zero), reference src/filters.jl:240): the materialised
        // input covers them; a direct source always has in_frames == need
        if (S.xscan) {  // exact scan between the state pass and the output pass
            double* vb = (double*)P->bufs[S.v_buf].d;
            double* sb = (double*)P->bufs[S.s0_buf].d;
            nl += launch_sos_phase(x, out.d, vb, nullptr, gg, S.groups[gi], 1, st);
            nl += launch_sos_xscan(vb, sb, (const double*)((char*)P->bufs[S.xs_mats_buf].d + gi * 2 * 16 * 16 * 8),
                                   (double*)P->bufs[S.sblk_buf].d, gg, S.groups[gi].nsec, st);
            nl += launch_sos_phase(x, out.d, nullptr, sb, gg, S.groups[gi], 3, st);
            continue;
        }
        nl += launch_sos(x, out.d, S.v_buf >= 0 ? (double*)P->bufs[S.v_buf].d : nullptr,
                         S.s0_buf >= 0 ? (double*)P->bufs[S.s0_buf].d : nullptr,
                         S.mpow_buf >= 0 ? (const double*)((char*)P->bufs[S.mpow_buf].d + gi * S.mpow_stride() * 8) : nullptr,
                         gg, S.groups[gi], st);
        nl += launch_sos_poison(out.d, gg, st);  // (behind a NaN the reference stays NaN: SosGeom::bad)
        if (gg.bad && gi + 1 < S.groups.size()) arm_bad(gg.bad, (size_t)N.nch, st);
    }
    return nl;
}

// the periodic resampler reads through its carriers; behind it, where a non-finite sample reached the accumulators, the
// launch that recomputes those outputs the reference's way
static void run_resample_periodic(Plan* P, const Step& s, const View& out, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    RsPeriodic rp = S.rp;
    rp.in_pitch = 0;
    rp.out_pitch = out.pitch;
    rp.out_f32 = s.idx == P->alias_stage && P->alias_narrow;
    if (rp.nstate > 0) {
        rp.wtab = (const double*)P->bufs[S.wtab_buf].d;
        rp.vper = (double*)P->bufs[S.vper_buf].d;
    }
    const int64_t al = 16 / (int64_t)dsize(N.dtype);
    rp.vec_ok = ((uintptr_t)out.d % 16 == 0) && (out.pitch % al == 0) && (rp.L % al == 0);
    static long long* d_trace = nullptr;  // SIGOPS_RS_TRACE tuning aid
    const bool tracing = std::getenv("SIGOPS_RS_TRACE") != nullptr;
    const size_t trace_n = (size_t)16 * kRsTraceIters * kRsTraceStamps;
    if (tracing) {
        if (!d_trace) HIPCHECK(hipMalloc(&d_trace, trace_n * 8));
        HIPCHECK(hipMemsetAsync(d_trace, 0, trace_n * 8, st));
        rp.trace = d_trace;
    }
    // (the list of (tile, group)s a non-finite sample reached, and the launch that recomputes them the reference's
    //  way: plain sources only -- a gain applied at the MFMA operand, a second array, a state pass keep the kernel's set)
    const bool nf_fix = S.rs_nf_buf >= 0 && S.rs_jrel_buf >= 0 && rp.ga == 0 && rp.arr2 == 0 && rp.nstate == 0 && S.ctl_buf >= 0 &&
                        S.car_buf >= 0 && !S.carriers.empty() && rp.rows <= 32 && rp.kw <= 160;
    rp.nf = nf_fix ? (uint32_t*)P->bufs[S.rs_nf_buf].d : nullptr;
    const double* tab = (const double*)P->bufs[S.tab_buf].d;
    const int* jend = (const int*)P->bufs[S.jend_buf].d;
    if (launch_resample_periodic(out.d, tab, jend, rp, N.dtype, global_tables(P, S), st) != 0)
        fail(SO_ERR_RUNTIME, "internal: no periodic resampler instantiation for this geometry");
    if (nf_fix) {
        RsPerFixup fx{};
        fx.g = rp;
        fx.tab = tab;
        fx.jend = jend;
        fx.jrel = (const int*)P->bufs[S.rs_jrel_buf].d;
        fx.taps = S.rg.taps;
        fx.out_f32 = (N.dtype == SO_F32 || rp.out_f32) ? 1 : 0;
        fx.gsrc = global_tables(P, S);
        fx.y = out.d;
        (void)launch_rs_fixup(fx, st);  // (a launch Step::launches has never counted: tests and recorded profiles pin the numbers)
    }
    if (tracing) dump_rs_trace(d_trace, trace_n, rp, st);
}

static int run_resample(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const View in = S.periodic ? View{nullptr, 0} : stage_in(P, S, N.nch, N.dtype), out = stage_out(P, s.idx, outp);
    const double* pfbt = S.tiled ? (const double*)P->bufs[S.pfbt_buf].d : nullptr;
    const double* dpfbt = S.tiled ? (const double*)P->bufs[S.dpfbt_buf].d : nullptr;
    if (S.periodic)
        run_resample_periodic(P, s, out, st);
    else if (S.rows) {
        RsRows rr = S.rr;
        rr.in_pitch = in.pitch;
        rr.out_pitch = out.pitch;
        if (std::getenv("SIGOPS_DEBUG_PLAN"))
            std::fprintf(stderr, "[sigops] k_resample_rows: ct=%d pb=%d tile_len=%d pitch=%d kw=%d ngroups=%d L=%lld M=%lld taps=%d\n", rr.ct, rr.pb,
                         rr.tile_len, rr.pitch, rr.kw, rr.ngroups, (long long)rr.L, (long long)rr.M, rr.taps);
        launch_resample_rows(in.d, out.d, (const double*)P->bufs[S.tab_buf].d, (const int*)P->bufs[S.jend_buf].d,
                             (const double*)P->bufs[S.mtab_buf].d, (const int*)P->bufs[S.mjend_buf].d, rr, N.dtype, st);
    } else if (S.tiled) {
        RsTiled rt = S.rt;
        rt.g.in_pitch = in.pitch;
        rt.g.out_pitch = out.pitch;
        bool done = false;
        if (S.arbk) {  // the persistent form, where it has an instantiation for the geometry
            RsArb ra = S.ra;
            ra.g.in_pitch = in.pitch;
            ra.g.out_pitch = out.pitch;
            ra.err = kernel_error_word(P);
            done = launch_resample_arb(in.d, out.d, pfbt, dpfbt, ra, st) == 0;
        }
        if (!done && rt.pair) launch_resample_tiled2(in.d, out.d, pfbt, dpfbt, rt, st);
        else if (!done) launch_resample_tiled(in.d, out.d, pfbt, dpfbt, rt, st);
    } else {
        RsGeom g = S.rg;
        g.in_pitch = in.pitch;
        g.out_pitch = out.pitch;
        launch_resample(in.d, out.d, (const double*)P->bufs[S.pfb_buf].d, (const double*)P->bufs[S.dpfb_buf].d, g, st);
    }
    if (S.fix_buf < 0) return 1;
    RsFixArgs fa{};  // the outputs DSP.jl's phase accumulator places differently
    fa.fix = (const RsFix*)P->bufs[S.fix_buf].d;
    fa.nfix = (int64_t)S.fix_host.size();
    fa.pfb = (const double*)P->bufs[S.pfb_buf].d;
    fa.dpfb = (const double*)P->bufs[S.dpfb_buf].d;
    fa.n_in = S.rg.n_in;
    fa.taps = S.rg.taps;
    fa.nch = N.nch;
    fa.stage_dtype = N.dtype;
    fa.out_dtype = (s.idx == P->alias_stage && P->alias_narrow) ? SO_F32 : N.dtype;
    if (S.periodic) {
        fa.car = (const DCarrier*)P->bufs[S.car_buf].d;
        fa.ncar = (int)S.carriers.size();
        fa.ops = P->d_ops;
        fa.leaves = P->d_leaves;
    } else {
        fa.x = in.d;
        fa.in_pitch = in.pitch;
        fa.in_dtype = N.dtype;
    }
    fa.y = out.d;
    fa.out_pitch = out.pitch;
    launch_resample_fix(fa, st);
    return 2;
}

// the sum of squares and the rms of it (two launches), over the stage's own buffer or, norm_direct, the array where it lies
static int run_norm(Plan* P, const Step& s, void* outp, hipStream_t st) {
    const Stage& S = P->stages[s.idx];
    const Node& N = P->nodes[S.node];
    const View v = S.norm_direct ? stage_in(P, S, N.nch, N.dtype) : stage_out(P, s.idx, outp);
    RmsPatch patch{};
    for (int li : S.rms_leaves) patch.dst[patch.n++] = &P->d_leaves[li].v0;
    launch_rms(v.d, N.dtype, S.need, N.nch, v.pitch, (double*)P->bufs[S.partial_buf].d, S.nparts, (double*)P->bufs[S.rms_buf].d, st, patch);
    return 2;
}

// Called from plan_execute ONLY, which sets Plan::graph_plan for the call: whether these launches may be captured into the
// plan's graph or stand next to its replays, and so must take the same arguments every time (run_rsos_fused: which set of
// `bad` words).  A caller that captures so_plan_execute into a graph of its OWN is not supported: a plan the executor
// does not replay itself alternates its sets from execute to execute, and a replay would not.
static int plan_execute_direct(Plan* P, void* outp, void* stream, std::string& err) {
    try {
        HIPCHECK(hipSetDevice(P->device));
        hipStream_t st = (hipStream_t)stream;
        if (P->out.nframes > 0 && !outp) fail(SO_ERR_INVALID, "so_plan_execute: null output");
        for (auto& h : P->host_leaves)
            if (h.bytes) HIPCHECK(hipMemcpyAsync(P->bufs[h.buf].d, P->array_ptr[h.node], h.bytes, hipMemcpyHostToDevice, st));
        // profiling 1: one set of events, read (after a synchronize) at the end of this execute;
        // profiling 2 (deferred): a set per execute, up to kProfExecs of them, nothing synchronised here --
        // so_plan_step_info averages them once the caller has synchronised (bench.py's timed region)
        const size_t evset = 2 * P->steps.size();
        const size_t pcap = prof_cap(P);
        const size_t evneed = P->profiling == 2 ? evset * pcap : evset;
        if (P->profiling && P->events.size() < evneed) {
            while (P->events.size() < evneed) {
                hipEvent_t e;
                HIPCHECK(hipEventCreate(&e));
                P->events.push_back(e);
            }
        }
        const size_t ev0 = P->profiling == 2 ? evset * ((size_t)P->prof_execs % pcap) : 0;
        if (P->out_alias_buf >= 0 && P->out.is_device && P->bufs[P->out_alias_buf].d != outp) {
            // in-place root pieces read the result: point their leaves at this execute's buffer
            P->bufs[P->out_alias_buf].d = outp;
            for (auto& L : P->leaves)
                if (L.buf == P->out_alias_buf) L.base = outp;
            if (P->d_leaves)
                HIPCHECK(hipMemcpyAsync(P->d_leaves, P->leaves.data(), P->leaves.size() * sizeof(DLeaf), hipMemcpyHostToDevice, st));
        }
        int launches = 0;
        // (profiling times the steps one after the other on the caller's stream)
        const bool lanes = P->nlanes > 1 && !P->profiling && !std::getenv("SIGOPS_RS_TRACE");
        hipStream_t const main_st = st;
        std::vector<char> lane_started(P->nlanes, 0);
        if (lanes) HIPCHECK(hipEventRecord(P->ev_start, main_st));  // after the H2D copies / earlier work
        for (size_t si = 0; si < P->steps.size(); ++si) {
            Step& s = P->steps[si];
            const int ln = lanes ? P->step_lane[si] : 0;
            hipStream_t st = ln == 0 ? main_st : P->lane_streams[ln];  // shadows the caller's stream
            if (lanes) {
                if (ln != 0 && !lane_started[ln]) {
                    HIPCHECK(hipStreamWaitEvent(st, P->ev_start, 0));
                    lane_started[ln] = 1;
                }
                for (int d : P->step_deps[si])
                    if (P->step_lane[d] != ln) HIPCHECK(hipStreamWaitEvent(st, P->step_done[d], 0));
            }
            if (P->profiling) HIPCHECK(hipEventRecord(P->events[ev0 + 2 * si], st));
            int nl = 0;
            switch (s.kind) {
            case 0: nl = run_pointwise(P, s, outp, st); break;
            case 2: nl = run_sos_batch(P, s, outp, st); break;
            case 3: nl = run_rsos_batch(P, s, outp, st); break;
            default:
                switch (P->stages[s.idx].kind) {
                case ST_SAMPLEAT: nl = run_sample_at(P, s, outp, st); break;
                case ST_COMB: nl = run_comb(P, s, outp, st); break;
                case ST_CUMSUM: nl = run_cumsum(P, s, outp, st); break;
                case ST_MOVING: nl = run_moving(P, s, outp, st); break;
                case ST_MOVSUM: nl = run_movsum(P, s, outp, st); break;
                case ST_MOVRANK: nl = run_movrank(P, s, outp, st); break;
                case ST_RECUR: nl = run_recur(P, s, outp, st); break;
                case ST_RECUR2: nl = run_recur2(P, s, outp, st); break;
                case ST_SOS: nl = run_sos(P, s, outp, st); break;
                case ST_RESAMPLE: nl = run_resample(P, s, outp, st); break;
                default: nl = run_norm(P, s, outp, st); break;
                }
            }
            s.launches = nl;
            launches += nl;
            if (P->profiling) HIPCHECK(hipEventRecord(P->events[ev0 + 2 * si + 1], st));
            if (lanes && (P->step_signals[si] || (ln != 0 && si + 1 == P->steps.size())))
                HIPCHECK(hipEventRecord(P->step_done[si], st));
        }
        if (lanes) {
            // join: everything the side lanes did is ordered before what follows on the caller's
            // stream (the last step of every side lane signals; wait for the last step per lane)
            std::vector<int> last(P->nlanes, -1);
            for (size_t si = 0; si < P->steps.size(); ++si) last[P->step_lane[si]] = (int)si;
            for (int l = 1; l < P->nlanes; ++l)
                if (last[l] >= 0) {
                    if (!P->step_signals[last[l]]) HIPCHECK(hipEventRecord(P->step_done[last[l]], P->lane_streams[l]));
                    HIPCHECK(hipStreamWaitEvent(main_st, P->step_done[last[l]], 0));
                }
        }
        HIPCHECK(hipGetLastError());
        P->stats.n_launches = launches;
        if (!P->out.is_device && P->out.nframes > 0) {
            Buf& b = P->bufs[P->out_stage_buf];
            size_t esz = dsize(P->out.dtype);
            bool planar = P->out.frame_stride == 1 && (P->out.nch == 1 || P->out.chan_stride == P->out.nframes);
            if (planar || P->interleaved_host) {
                HIPCHECK(hipMemcpyAsync(outp, b.d, b.bytes, hipMemcpyDeviceToHost, st));
                HIPCHECK(hipStreamSynchronize(st));
            } else {
                P->host_tmp.resize(b.bytes);
                HIPCHECK(hipMemcpyAsync(P->host_tmp.data(), b.d, b.bytes, hipMemcpyDeviceToHost, st));
                HIPCHECK(hipStreamSynchronize(st));
                for (int c = 0; c < P->out.nch; ++c)
                    for (int64_t f = 0; f < P->out.nframes; ++f)
                        std::memcpy((char*)outp + (size_t)(f * P->out.frame_stride + c * P->out.chan_stride) * esz,
                                    P->host_tmp.data() + (size_t)(c * P->out.nframes + f) * esz, esz);
            }
        } else if (!P->host_leaves.empty() || P->profiling == 1) {
            HIPCHECK(hipStreamSynchronize(st));
        }
        if (!P->out.is_device && P->out.nframes > 0) {  // (synchronised above)
            std::string why;
            if (kernel_gave_up(P, why)) fail(SO_ERR_RUNTIME, why);
        }
        if (P->profiling == 2) P->prof_execs++;
        if (P->profiling == 1) {
            HIPCHECK(hipStreamSynchronize(st));
            double total = 0, best = -1;
            for (size_t si = 0; si < P->steps.size(); ++si) {
                float ms = 0;
                HIPCHECK(hipEventElapsedTime(&ms, P->events[2 * si], P->events[2 * si + 1]));
                P->steps[si].ms = ms;
                total += ms;
                if (ms > best) {
                    best = ms;
                    P->stats.dominant_kernel_ms = ms;
                    P->stats.dominant_kernel_bytes = P->steps[si].bytes;
                    std::snprintf(P->stats.dominant_kernel, sizeof P->stats.dominant_kernel, "%s", P->steps[si].name.c_str());
                }
            }
            P->stats.last_exec_ms = total;
        }
    } catch (const PlanError& e) {
        disarm_bad(P);
        err = e.msg;
        return e.status;
    }
    return SO_OK;
}

// so_plan_execute.  Plans with many small launches (config 4: 33 launches and ~40 event
// operations per execute) are host-bound, so from the second execute with the same result
// pointer on, the whole multi-stream launch sequence is replayed from a captured HIP graph.
int plan_execute(Plan* P, void* outp, void* stream, std::string& err) {
    DeviceGuard guard(P->device);
    if (kernel_gave_up(P, err)) {
        disarm_bad(P);
        return SO_ERR_RUNTIME;
    }
    const bool eligible = P->steps.size() >= 4 && P->out.is_device && P->host_leaves.empty() && !P->profiling &&
                          !std::getenv("SIGOPS_NO_GRAPH") && !std::getenv("SIGOPS_RS_TRACE");
    P->graph_plan = eligible;
    if (!eligible) {
        P->n_direct++;
        return plan_execute_direct(P, outp, stream, err);
    }
    hipStream_t st = (hipStream_t)stream;
    // The captured launches read the leaf table on the device as it stood at capture time.  In-place root
    // pieces read the RESULT through leaves that plan_execute_direct re-points at every new result
    // pointer: after a direct execute into another buffer the table no longer matches the graph (A, A,
    // B, A would apply the in-place gains to B's values a second time), so the graph is only replayed
    // while those leaves still point at its buffer; otherwise this execute goes the direct way, which
    // points them back.
    const bool leaves_match = P->out_alias_buf < 0 || P->bufs[P->out_alias_buf].d == outp;
    if (P->graph_exec && P->graph_out == outp && P->graph_epoch == P->array_epoch && leaves_match) {
        if (hipSetDevice(P->device) == hipSuccess && hipGraphLaunch(P->graph_exec, st) == hipSuccess) {
            P->n_replays++;
            return SO_OK;
        }
        (void)hipGetLastError();
        (void)hipGraphExecDestroy(P->graph_exec);  // fall back to direct launches for good
        P->graph_exec = nullptr;
        P->graph_failed = true;
    }
    if (P->graph_failed || P->last_out != outp || P->last_epoch != P->array_epoch) {
        // first execute for this result / these arrays: plain launches (also performs the
        // one-time function attribute calls, which must not happen inside a capture)
        P->last_out = outp;
        P->last_epoch = P->array_epoch;
        P->n_direct++;
        return plan_execute_direct(P, outp, stream, err);
    }
    if (P->graph_exec && P->graph_out == outp && P->graph_epoch == P->array_epoch) {
        // (the graph is still the right one; only the leaf table had moved)
        P->n_direct++;
        return plan_execute_direct(P, outp, stream, err);
    }
    if (P->graph_exec) {
        (void)hipGraphExecDestroy(P->graph_exec);
        P->graph_exec = nullptr;
    }
    hipGraph_t graph = nullptr;
    // capture on a stream of our own (the caller's may be the legacy default stream, which cannot
    // be captured); the graph is then launched on the caller's stream
    if (!P->capture_stream && hipStreamCreateWithFlags(&P->capture_stream, hipStreamNonBlocking) != hipSuccess)
        P->capture_stream = nullptr;
    if (!P->capture_stream || hipSetDevice(P->device) != hipSuccess ||
        hipStreamBeginCapture(P->capture_stream, hipStreamCaptureModeRelaxed) != hipSuccess) {
        (void)hipGetLastError();
        P->graph_failed = true;
        return plan_execute_direct(P, outp, stream, err);
    }
    const int rc = plan_execute_direct(P, outp, (void*)P->capture_stream, err);
    const hipError_t ec = hipStreamEndCapture(P->capture_stream, &graph);
    if (std::getenv("SIGOPS_DEBUG_PLAN"))
        std::fprintf(stderr, "[sigops] graph capture: rc=%d end=%d (%s) graph=%p err=%s\n", rc, (int)ec, hipGetErrorString(ec), (void*)graph, err.c_str());
    if (rc != SO_OK || ec != hipSuccess || !graph ||
        hipGraphInstantiate(&P->graph_exec, graph, nullptr, nullptr, 0) != hipSuccess) {
        (void)hipGetLastError();
        if (graph) (void)hipGraphDestroy(graph);
        P->graph_exec = nullptr;
        P->graph_failed = true;
        return rc != SO_OK ? rc : plan_execute_direct(P, outp, stream, err);
    }
    (void)hipGraphDestroy(graph);
    P->graph_out = outp;
    P->graph_epoch = P->array_epoch;
    P->n_captures++;
    if (hipGraphLaunch(P->graph_exec, st) != hipSuccess) {
        (void)hipGetLastError();
        P->graph_failed = true;
        return plan_execute_direct(P, outp, stream, err);
    }
    return SO_OK;
}

int plan_set_array(Plan* P, int32_t node_index, const void* data, std::string& err) {
    if (node_index < 0 || node_index >= (int)P->nodes.size() || P->nodes[node_index].nd.kind != SO_NODE_ARRAY) {
        err = "so_plan_set_array: not an ARRAY node";
        return SO_ERR_INVALID;
    }
    DeviceGuard guard(P->device);
    P->array_ptr[node_index] = data;
    P->array_epoch++;  // invalidates a captured launch graph
    if (P->nodes[node_index].nd.i0) {  // device leaf: patch the leaf table
        bool changed = false;
        for (size_t i = 0; i < P->leaves.size(); ++i)
            if (P->leaf_array_node[i] == node_index) {
                P->leaves[i].base = data;
                changed = true;
            }
        if (changed && P->d_leaves)
            if (hipMemcpy(P->d_leaves, P->leaves.data(), P->leaves.size() * sizeof(DLeaf), hipMemcpyHostToDevice) != hipSuccess) {
                err = "so_plan_set_array: leaf upload failed";
                return SO_ERR_RUNTIME;
            }
        // carriers of fused resampler stages (by value at launch + a device copy for the slow path)
        for (auto& S : P->stages) {
            bool touched = false;
            for (auto& c : S.carriers) {
                if (c.array_node == node_index) {
                    c.base = data;
                    const int64_t V = 16 / (int64_t)dsize(c.dtype);
                    c.vec_ok = carrier_vec_ok(c, V);
                    touched = true;
                }
                if (car_has_arr2(c) && c.array_node2 == node_index) {
                    c.base2 = data;
                    c.vec_ok2 = (uintptr_t)c.base2 % (c.dtype2 == SO_F64 ? 8 : 4) == 0;
                    touched = true;
                }
            }
            if (touched) {
                const RsCtl ctl = P->make_ctl(S);
                if (hipMemcpy(P->bufs[S.car_buf].d, S.carriers.data(), S.carriers.size() * sizeof(DCarrier), hipMemcpyHostToDevice) != hipSuccess ||
                    hipMemcpy(P->bufs[S.ctl_buf].d, &ctl, sizeof(RsCtl), hipMemcpyHostToDevice) != hipSuccess) {
                    err = "so_plan_set_array: carrier upload failed";
                    return SO_ERR_RUNTIME;
                }
            }
        }
    }
    return SO_OK;
}

int64_t plan_nframes(const Plan* P) {
    const Node& R = P->nodes[P->root];
    return isinf_(R.len) ? SO_LEN_INF : R.len.n;
}
void plan_stats(const Plan* P, so_stats_t* st) { *st = P->stats; }
void plan_set_profiling(Plan* P, int mode) {
    P->profiling = mode < 0 || mode > 2 ? 1 : mode;
    P->prof_execs = 0;
}
int64_t plan_counter(const Plan* P, int which) {
    switch (which) {
    case SO_COUNTER_GRAPH_REPLAYS: return P->n_replays;
    case SO_COUNTER_GRAPH_CAPTURES: return P->n_captures;
    case SO_COUNTER_DIRECT_EXECUTES: return P->n_direct;
    case SO_COUNTER_FUSED_MFMAS_PER_BLOCK: {  // k_rsos: window k-steps + 14 (D . X, X^T T^T, the chain's A^16 . S, S^T C^T)
        for (const Stage& S : P->stages)    // ... + 10 for a folded plan (E . Z, the chain's A^16 . S, C . S)
                                            // (the chain's share counts as three large MFMAs whatever shape it runs on)
            if (S.kind == ST_SOS && S.rsos_src >= 0 && S.need > 0) return S.rs.ks + (S.rs.fold ? 10 : 14);
        return 0;
    }
    case SO_COUNTER_RSOS_FOLD: {  // k_rsos: the folded block (RsSos::fold)
        for (const Stage& S : P->stages)
            if (S.kind == ST_SOS && S.rsos_src >= 0 && S.need > 0) return S.rs.fold;
        return 0;
    }
    case SO_COUNTER_RSOS_CHAIN4: {  // k_rsos: the chain's recurrence on the 4 x 4 x 4 shape (RsSos::chain4_off)
        for (const Stage& S : P->stages)
            if (S.kind == ST_SOS && S.rsos_src >= 0 && S.need > 0) return S.rs.chain4_off != 0 ? 1 : 0;
        return 0;
    }
    case SO_COUNTER_WPROJ: {  // k_rsos: the warm-up of a range as one product where it lies inside the array (RsSos::wproj)
        for (const Stage& S : P->stages)
            if (S.kind == ST_SOS && S.rsos_src >= 0 && S.need > 0) return S.rs.wproj;
        return 0;
    }
    case SO_COUNTER_RSOS_RANGE_PERIODS:
    case SO_COUNTER_RSOS_WARMUP_PERIODS:
    case SO_COUNTER_RSOS_PERIOD_INPUTS:
    case SO_COUNTER_WPROJ_FRAMES:
    case SO_COUNTER_WPROJ_FIRST:
        for (const Stage& S : P->stages)
            if (S.kind == ST_SOS && S.rsos_src >= 0 && S.need > 0)
                return which == SO_COUNTER_RSOS_RANGE_PERIODS ? S.rs.pr : which == SO_COUNTER_RSOS_WARMUP_PERIODS ? S.rs.wp
                     : which == SO_COUNTER_RSOS_PERIOD_INPUTS ? S.rs.M : which == SO_COUNTER_WPROJ_FRAMES ? S.rs.wk : S.rs.wj0;
        return 0;
    default: break;
    }
    // the nodes that carry a stream's state, in node-table order: how many, which, and where their carry-out records stand
    const int64_t nc = (int64_t)P->carry_nodes.size();
    if (which == SO_COUNTER_CARRY_NODES) return nc;
    for (const int64_t first : {(int64_t)SO_COUNTER_CARRY_NODE_FIRST, (int64_t)SO_COUNTER_CARRY_FRAME_FIRST, (int64_t)SO_COUNTER_CARRY_NEED_FIRST}) {
        if (which < first || which >= first + nc) continue;
        const int ni = P->carry_nodes[(size_t)(which - first)];
        if (first == SO_COUNTER_CARRY_NODE_FIRST) return ni;
        for (const Stage& S : P->stages)
            if (S.node == ni && S.processed) return first == SO_COUNTER_CARRY_NEED_FIRST ? S.need : S.carried;
        return first == SO_COUNTER_CARRY_NEED_FIRST ? 0 : P->nodes[ni].nd.s0;  // (nobody reads the node: nothing ran)
    }
    return -1;
}
int plan_step_info(const Plan* P, int index, so_step_info_t* info) {
    if (info && index >= 0 && index < (int)P->steps.size()) {
        const Step& s = P->steps[index];
        std::memset(info, 0, sizeof *info);
        std::snprintf(info->name, sizeof info->name, "%s", s.name.c_str());
        info->algorithmic_bytes = s.bytes;
        info->ms = s.ms;
        if (P->profiling == 2 && P->prof_execs > 0) {
            // deferred mode: mean over the (up to kProfExecs most recent) executes recorded since
            // so_plan_set_profiling(plan, 2); the caller has synchronised the stream
            const size_t evset = 2 * P->steps.size();
            const int64_t n = std::min<int64_t>(P->prof_execs, (int64_t)prof_cap(P));
            double sum = 0;
            int64_t got = 0;
            for (int64_t e = 0; e < n; ++e) {
                float ms = 0;
                if (hipEventElapsedTime(&ms, P->events[evset * e + 2 * index], P->events[evset * e + 2 * index + 1]) == hipSuccess) {
                    sum += ms;
                    ++got;
                } else (void)hipGetLastError();
            }
            info->ms = got ? sum / (double)got : 0.0;
        }
        info->launches = s.launches;
    }
    return (int)P->steps.size();
}
// so_plan_check: waits for everything the plan has launched so far (the stream its last execute ran on -- or the whole
// device where the plan ran on lanes of its own) and reports what only shows once the kernels have run: a kernel that
// gave up on a wait between its waves.  The call a host makes behind an execute into a DEVICE result before it trusts it
// (a host result's execute synchronises and reports by itself).
int plan_check(Plan* P, void* stream, std::string& err) {
    DeviceGuard guard(P->device);
    try {
        if (P->nlanes > 1 || P->graph_exec) HIPCHECK(hipDeviceSynchronize());
        else HIPCHECK(hipStreamSynchronize((hipStream_t)stream));
    } catch (const PlanError& e) {
        err = e.msg;
        return e.status;
    }
    if (kernel_gave_up(P, err)) return SO_ERR_RUNTIME;
    return SO_OK;
}

void plan_destroy(Plan* P) {
    if (!P) return;
    {
        DeviceGuard guard(P->device);
        P->release();
    }
    delete P;
}


}  // namespace so
