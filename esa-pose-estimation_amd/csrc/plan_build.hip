// plan_build.hip — configuration and plan switches -> the static plan of a handle (esahrnet_create): the op list over the plan's
// tensors, its multi-head and job groups, the wave schedule, and the fp16 scale groups read off it.  No shape, no device memory.
#include "plan.h"

namespace esa {

PlanOptions plan_options(const esahrnet_cfg& g, const esa::Format& format) {
    const auto on = esa::env_on;
    PlanOptions o;
    o.unfused = on("ESAHRNET_UNFUSED"); o.head_v1 = on("ESAHRNET_HEAD_V1"); o.final_valu = on("ESAHRNET_FINAL_VALU");
    o.no_multihead = on("ESAHRNET_NO_MULTIHEAD"); o.no_jobs = on("ESAHRNET_NO_JOBS"); o.no_bblock = on("ESAHRNET_NO_BBLOCK");
    o.no_cbam_jobs = on("ESAHRNET_NO_CBAM_JOBS"); o.cbam_unfused = on("ESAHRNET_CBAM_UNFUSED");
    o.stem_pool_separate = on("ESAHRNET_STEM_POOL_SEPARATE"); o.head3_direct = on("ESAHRNET_HEAD3_DIRECT");
    o.head3_cout32 = on("ESAHRNET_HEAD3_COUT32"); o.bf_unfused_head = on("ESAHRNET_BF_UNFUSED_HEAD");
    o.bf_head_valu = on("ESAHRNET_BF_HEAD_VALU"); o.x6_unfused_head = on("ESAHRNET_X6_UNFUSED_HEAD");
    o.x6_unfused_stem = on("ESAHRNET_X6_UNFUSED_STEM"); o.tap_all = on("ESAHRNET_TAP_ALL");
    o.x6_reload_weights = on("ESAHRNET_X6_RELOAD_WEIGHTS");     // (changes no op: the same launches, the same names)
    const char* streams = getenv("ESAHRNET_STREAMS");
    o.nlanes = streams && atoi(streams) > 1 ? 4 : 1;
    o.fmt = format.fmt;
    const bool sb = o.fmt == esa::FMT_SB, v0 = g.variant == 0;
    // the fused stem kernels: stem_fused serves every (cin, stem width) in the split format, stem_x6_kernel one; none in bf16
    const bool x6_stem = esa::stem_fused_x6_supported(g.cin, pad32(g.stem_width), pad32(g.stem_width)) && g.stem_width == 64;
    o.stem = sb && (!v0 || !o.unfused) ? STEM_FUSED
           : o.fmt == esa::FMT_F32 && x6_stem && !o.x6_unfused_stem ? STEM_FUSED_X6 : STEM_SEPARATE;
    // bblock32 is built for the split format, and seg_hrnet3's block has a CBAM inside
    o.fused_block = sb && v0 && !o.unfused && !o.no_bblock;
    int nb4 = 0;                // branches of stage 4
    while (nb4 < ESAHRNET_MAX_BRANCHES && g.blocks[3][nb4] > 0) ++nb4;
    const int c0 = pad32(g.widths[0]);
    o.head = !v0 || nb4 != 4 ? HEAD_UNFUSED
           : sb ? (!o.unfused && (c0 == 32 || c0 == 64) ? HEAD_SB : HEAD_UNFUSED)
           : esa::fmt_half(o.fmt) ? (!o.bf_unfused_head && (pad64(g.widths[0]) == 64 || pad64(g.widths[0]) == 128) ? HEAD_BF : HEAD_UNFUSED)
           : !o.x6_unfused_head && (c0 == 32 || c0 == 64) ? HEAD_X6 : HEAD_UNFUSED;
    // head_fused2 needs head_t's channel counts on branches 2 and 3 and 64 or 96 on branch 1
    o.head2 = !o.head_v1 && (o.head != HEAD_SB || ((pad32(g.widths[1]) == 64 || pad32(g.widths[1]) == 96) &&
                                                   esa::head_t_supported(pad32(g.widths[2])) && esa::head_t_supported(pad32(g.widths[3]))));
    o.final_mfma = v0 && o.fmt != esa::FMT_F32 && !o.final_valu && esa::final_mfma_supported(g.num_keypoints, g.cin);
    return o;
}

namespace {

struct Builder {
    esahrnet_ctx& c;
    int jkey = -1;              // job key given to the next stride-1 convolutions (HRModule branches), -1: none
    int jkey2 = -1;             // job key given to the next stride-2 convolution (fuse-down chain link), -1: none
    explicit Builder(esahrnet_ctx& ctx) : c(ctx) {}

    int spec(const std::string& name, const std::string& bn, int cin, int cout, int k, int stride,
             int level, bool bias, bool relu) {
        ConvSpec s;
        s.name = name; s.bn = bn; s.cin = cin; s.cout = cout; s.k = k; s.stride = stride;
        s.level = level; s.has_bias = bias; s.relu = relu;
        c.specs.push_back(s);
        c.spec_by_name[name] = (int)c.specs.size() - 1;
        c.max_level = std::max(c.max_level, level);
        return (int)c.specs.size() - 1;
    }
    int taps_spec(int parent, int c0, int c1, int level) {
        const std::string name = c.specs[parent].name + "#taps[" + std::to_string(c0) + ":" + std::to_string(c1) + "]";
        const int cout9 = 9 * ((c.specs[parent].cout + 7) & ~7);
        const int sp = spec(name, "", c1 - c0, cout9, 1, 1, level, false, false);
        c.specs[sp].parent = parent; c.specs[sp].pc0 = c0; c.specs[sp].pc1 = c1;
        if (c.nhost_specs < 0) c.nhost_specs = sp;
        return sp;
    }
    int tensor(int C, int level, const std::string& tap = "") {
        Tensor t;
        t.C = C; t.Cp = c.padc(C); t.level = level; t.tap = tap; t.key = tap;
        c.tensors.push_back(t);
        return (int)c.tensors.size() - 1;
    }
    void use(int t, int op) {
        if (t < 0) return;
        c.tensors[t].last = std::max(c.tensors[t].last, op);
    }
    // conv op on a spec (optionally a cin slice, optionally plain-f32 output); returns the output tensor
    int conv(int sp, int in, int res, bool relu, const std::string& tap = "", int c0 = 0, int c1 = -1,
             bool use_bias = true, bool out_f32 = false) {
        const ConvSpec& s = c.specs[sp];
        DevConv d;
        d.spec = sp; d.c0 = c0; d.c1 = c1 < 0 ? s.cin : c1; d.use_bias = use_bias; d.out_f32 = out_f32;
        d.cinp = c.padc(d.c1 - d.c0); d.coutp = c.padc(s.cout);
        c.dconvs.push_back(d);
        Op o;
        o.kind = OP_CONV; o.dconv = (int)c.dconvs.size() - 1; o.in = in; o.res = res; o.relu = relu;
        if (jkey >= 0 && s.k == 3 && s.stride == 1) o.jkey = jkey++;
        if (jkey2 >= 0 && ((s.k == 3 && s.stride == 2) || s.k == 1)) o.jkey = jkey2;
        // ESAHRNET_TAP_ALL=1 (debugging): every convolution output becomes a named tap
        o.out = tensor(s.cout, s.level, tap.empty() && !out_f32 && c.opt.tap_all ? "conv:" + s.name : tap);
        c.tensors[o.out].f32 = out_f32;
        c.tensors[o.out].key = !tap.empty() ? tap : d.c0 != 0 || d.c1 != s.cin
            ? s.name + "[:, " + std::to_string(d.c0) + ":" + std::to_string(d.c1) + "]" : s.name;
        const int idx = (int)c.ops.size();
        c.tensors[o.out].def = idx;
        use(in, idx); use(res, idx);
        c.ops.push_back(o);
        return o.out;
    }
    int fuse(const std::vector<int>& terms, int C, int level, bool relu, const std::string& tap = "", const std::string& key = "") {
        Op o;
        o.kind = OP_FUSE; o.nterms = (int)terms.size(); o.relu = relu;
        o.out = tensor(C, level, tap);
        if (tap.empty()) c.tensors[o.out].key = key;
        const int idx = (int)c.ops.size();
        c.tensors[o.out].def = idx;
        for (int i = 0; i < o.nterms; ++i) { o.terms[i] = terms[i]; use(terms[i], idx); }
        c.ops.push_back(o);
        return o.out;
    }
    int aux(const std::string& name, int a, int b, int kh, int kw) {
        AuxSpec s;
        s.name = name; s.shape[0] = a; s.shape[1] = b; s.shape[2] = kh; s.shape[3] = kw;
        c.aux.push_back(s);
        return (int)c.aux.size() - 1;
    }
    int push(Op& o) {
        const int idx = (int)c.ops.size();
        if (o.out >= 0 && c.tensors[o.out].def < 0) c.tensors[o.out].def = idx;
        use(o.in, idx); use(o.res, idx);
        for (int i = 0; i < 4; ++i) use(o.terms[i], idx);
        c.ops.push_back(o);
        return idx;
    }
    int flat_tensor(int floats_per_sample) {
        Tensor t;
        t.C = t.Cp = 0; t.level = 0; t.flat = floats_per_sample;
        c.tensors.push_back(t);
        return (int)c.tensors.size() - 1;
    }
    // CBAM (seg_hrnet3.py:32-61, 90-91): y[:, c0:c0+C] = [relu]( sa(ca*x) * (ca*x) [+ res] ); prefix p
    // names the owner of .ca / .sa ("" = the network's own).  Returns nothing: writes into `y`.
    void cbam(const std::string& p, int x, int C, int res, bool relu, int y, int y_c0) {
        const std::string q = p.empty() ? "" : p + ".";
        const int cr = C / 16;
        const int a0 = aux(q + "ca.fc.0.weight", cr, C, 1, 1), a1 = aux(q + "ca.fc.2.weight", C, cr, 1, 1);
        const int a2 = aux(q + "sa.conv1.weight", 1, 2, 7, 7);
        const int level = c.tensors[x].level, Cp = c.tensors[x].Cp;
        const int partial = flat_tensor(esa::POOL_SLABS * Cp * 2), cav = flat_tensor(Cp);
        Tensor mt; mt.C = 2; mt.Cp = 2; mt.level = level; mt.f32 = true;       // (f32 [N][H][W][2] in every format)
        mt.key = q + "sa.maps";
        c.tensors.push_back(mt);
        const int maps = (int)c.tensors.size() - 1;
        // inside an HRModule branch (jkey >= 0) the four CBAM launches take the next depth keys behind the block's two
        // convolutions, so that group_jobs can put the module in depth-major order and merge the convolutions of its branches
        auto key = [&]() { return jkey >= 0 ? jkey++ : -1; };
        { Op o; o.kind = OP_POOL; o.in = x; o.out = partial; o.aux[0] = a0; o.jkey = key(); push(o); }
        { Op o; o.kind = OP_MLP; o.in = partial; o.out = cav; o.aux[0] = a0; o.aux[1] = a1; o.nchan = C; o.terms[0] = x; o.jkey = key(); push(o); }
        { Op o; o.kind = OP_MAPS; o.in = x; o.terms[1] = cav; o.out = maps; o.aux[0] = a0; o.nchan = C; o.jkey = key(); push(o); }
        { Op o; o.kind = OP_APPLY; o.in = x; o.res = res; o.terms[1] = cav; o.terms[2] = maps; o.aux[0] = a0; o.aux[2] = a2;
          o.out = y; o.c0 = y_c0; o.relu = relu; o.nchan = C; o.jkey = key(); push(o); }
    }
    // BasicBlock of seg_hrnet3.py:64-103: conv-bn-relu-conv-bn, CBAM, (+res), relu
    int basic_block_cbam(const std::string& p, int x, int cin, int cout, int level, const std::string& tap) {
        int res = x;
        const int c1 = spec(p + ".conv1", p + ".bn1", cin, cout, 3, 1, level, false, true);
        const int c2 = spec(p + ".conv2", p + ".bn2", cout, cout, 3, 1, level, false, false);
        if (cin != cout) {
            const int d = spec(p + ".downsample.0", p + ".downsample.1", cin, cout, 1, 1, level, false, false);
            res = conv(d, x, -1, false);
        }
        const int o1 = conv(c1, x, -1, true);
        const int o2 = conv(c2, o1, -1, false);
        const int y = tensor(cout, level, tap);
        if (tap.empty()) c.tensors[y].key = p + ".cbam";
        cbam(p, o2, cout, res, true, y, 0);
        return y;
    }
    // BasicBlock (seg_hrnet.py:32-61): conv-bn-relu-conv-bn (+res) relu
    int basic_block(const std::string& p, int x, int cin, int cout, int level, const std::string& tap) {
        if (c.cfg.variant == 1) return basic_block_cbam(p, x, cin, cout, level, tap);
        int res = x;
        const int c1 = spec(p + ".conv1", p + ".bn1", cin, cout, 3, 1, level, false, true);
        const int c2 = spec(p + ".conv2", p + ".bn2", cout, cout, 3, 1, level, false, true);
        // whole block in one kernel (bblock32.hip) — for layer1; inside the HRModules the block's two convolutions join the
        // same-depth convolutions of the other branches in one launch instead (group_jobs; ESAHRNET_NO_JOBS=1: fused block)
        const bool in_job = jkey >= 0 && !c.opt.no_jobs;
        if (c.opt.fused_block && cin == cout && pad32(cin) == 32 && !in_job) {
            Op o;
            o.kind = OP_BLOCK; o.in = x; o.relu = true;
            for (int k = 0; k < 2; ++k) {
                DevConv d;
                d.spec = k ? c2 : c1; d.c0 = 0; d.c1 = cin; d.use_bias = true; d.cinp = 32; d.coutp = 32;
                c.dconvs.push_back(d);
                (k ? o.dconv2 : o.dconv) = (int)c.dconvs.size() - 1;
            }
            o.out = tensor(cout, level, tap);
            if (tap.empty()) c.tensors[o.out].key = c.specs[c2].name;
            const int idx = (int)c.ops.size();
            c.tensors[o.out].def = idx;
            use(x, idx);
            c.ops.push_back(o);
            return o.out;
        }
        if (cin != cout) {
            const int d = spec(p + ".downsample.0", p + ".downsample.1", cin, cout, 1, 1, level, false, false);
            res = conv(d, x, -1, false);
        }
        const int o = conv(c1, x, -1, true);
        return conv(c2, o, res, true, tap);
    }
};

// Post-pass over the op list: find the stride-2 3x3 convolutions that share their input and make each such group
// consecutive (moving a member EARLIER is always legal: its only input is defined before the group's first member).
void group_multihead(esahrnet_ctx& c) {
    if (c.opt.no_multihead || c.opt.fmt != esa::FMT_SB) return;
    auto eligible = [&](const Op& o) {
        if (o.kind != OP_CONV || o.res >= 0 || o.alt != 0 || o.multi >= 0) return false;
        const DevConv& d = c.dconvs[o.dconv];
        const ConvSpec& s = c.specs[d.spec];
        return s.k == 3 && s.stride == 2 && !d.out_f32 && d.c0 == 0 && d.c1 == s.cin && d.perm.empty() && d.use_bias;
    };
    std::vector<Op> ops = c.ops;
    for (size_t i = 0; i < ops.size(); ++i) {
        if (!eligible(ops[i])) continue;
        std::vector<size_t> members{i};
        for (size_t j = i + 1; j < ops.size() && members.size() < 3; ++j)
            if (eligible(ops[j]) && ops[j].in == ops[i].in) members.push_back(j);
        if (members.size() < 2) continue;
        // measured (W32, batch 32): worth it only where the shared input is the big 32/48-channel branch AND the
        // heads add up to whole 64-cout workgroup slices (stage 4: 53.4 -> 40.8 us); 96 couts on 32-cout slices
        // (stage 3: 40.1 -> 45.2 us) and the 64-channel input (31.8 -> 32.6 us) are not
        {
            int tot = 0;
            for (size_t k : members) tot += c.dconvs[ops[k].dconv].coutp;
            if (tot % 64 != 0 || c.dconvs[ops[i].dconv].cinp > 64 || c.tensors[ops[i].in].level > 1) continue;
        }
        const int mi = (int)c.multis.size();
        Multi m;
        m.n = (int)members.size();
        // pull the members up behind the leader (back to front so that the indices stay valid)
        std::vector<Op> pulled;
        for (size_t k = members.size(); k-- > 1;) {
            pulled.insert(pulled.begin(), ops[members[k]]);
            ops.erase(ops.begin() + members[k]);
        }
        ops.insert(ops.begin() + i + 1, pulled.begin(), pulled.end());
        for (int k = 0; k < m.n; ++k) {
            ops[i + k].multi = mi;
            ops[i + k].mpos = k;
            m.op[k] = (int)(i + k);
            m.coutp += c.dconvs[ops[i + k].dconv].coutp;
        }
        c.multis.push_back(m);
    }
    c.ops = ops;
    // op indices moved: recompute first definition / last use of every tensor and the head2 op index
    for (Tensor& t : c.tensors) { t.def = -1; t.last = -1; }
    c.head2_op = -1;
    for (size_t k = 0; k < c.ops.size(); ++k) {
        const Op& o = c.ops[k];
        if (o.kind == OP_HEAD2) c.head2_op = (int)k;
        if (o.out >= 0 && c.tensors[o.out].def < 0) c.tensors[o.out].def = (int)k;
        if (o.out2 >= 0 && c.tensors[o.out2].def < 0) c.tensors[o.out2].def = (int)k;
        auto use = [&](int t) { if (t >= 0) c.tensors[t].last = std::max(c.tensors[t].last, (int)k); };
        use(o.in); use(o.res);
        for (int t = 0; t < 4; ++t) use(o.terms[t]);
    }
}

// Post-pass: inside one HRModule the branches are independent chains of 3x3 convolutions.  The builder emits them
// branch by branch; here the convolutions of a module are put in depth-major order (stable, so every branch keeps its own
// order) and the same-depth ones of up to three branches become a JobGroup.
void group_jobs(esahrnet_ctx& c) {
    if (c.opt.no_jobs) return;
    std::vector<Op> ops = c.ops;
    auto eligible = [&](const Op& o) {
        // the CBAM launches of a depth (seg_hrnet3): same kind on every branch, one launch (cbam.hip: cbam_jobs_kernel)
        if ((o.kind == OP_POOL || o.kind == OP_MLP || o.kind == OP_MAPS || o.kind == OP_APPLY) && o.jkey >= 0)
            return !c.opt.no_cbam_jobs;
        if (o.kind != OP_CONV || o.jkey < 0 || o.alt != 0 || o.multi >= 0) return false;
        const DevConv& d = c.dconvs[o.dconv];
        const ConvSpec& s = c.specs[d.spec];
        if (s.k == 1) return !c.h16() && o.res < 0 && !d.out_f32 && d.c0 == 0 && d.c1 == s.cin && d.perm.empty() && d.use_bias;
        return s.k == 3 && !d.out_f32 && d.c0 == 0 && d.c1 == s.cin && d.perm.empty() && d.use_bias &&
               d.coutp % (c.h16() ? 64 : 32) == 0;
    };
    size_t i = 0;
    while (i < ops.size()) {
        if (ops[i].jkey < 0) { ++i; continue; }
        const int mod = ops[i].jkey >> 8;
        size_t j = i;
        while (j < ops.size() && ops[j].jkey >= 0 && (ops[j].jkey >> 8) == mod) ++j;      // [i, j): this module's branch convs
        std::stable_sort(ops.begin() + i, ops.begin() + j, [](const Op& a, const Op& b) { return (a.jkey & 255) < (b.jkey & 255); });
        for (size_t a = i; a < j;) {
            size_t b = a;
            std::vector<size_t> mem;
            const size_t cap = ops[a].kind == OP_CONV && c.specs[c.dconvs[ops[a].dconv].spec].k == 1 ? 6 : 4;
            while (b < j && ops[b].jkey == ops[a].jkey) { if (eligible(ops[b]) && mem.size() < cap) mem.push_back(b); ++b; }
            // members must be consecutive for the leader to stand for them: move the ineligible ones of this depth behind
            if (mem.size() >= 2) {
                std::vector<Op> grp, rest;
                for (size_t k = a; k < b; ++k) (std::find(mem.begin(), mem.end(), k) != mem.end() ? grp : rest).push_back(ops[k]);
                JobGroup g;
                g.n = (int)grp.size();
                for (int k = 0; k < g.n; ++k) { grp[k].job = (int)c.jobs.size(); grp[k].jpos = k; g.op[k] = (int)(a + k); }
                std::copy(grp.begin(), grp.end(), ops.begin() + a);
                std::copy(rest.begin(), rest.end(), ops.begin() + a + grp.size());
                c.jobs.push_back(g);
            }
            a = b;
        }
        i = j;
    }
    c.ops = ops;
    for (Tensor& t : c.tensors) { t.def = -1; t.last = -1; }
    c.head2_op = -1;
    for (size_t k = 0; k < c.ops.size(); ++k) {
        const Op& o = c.ops[k];
        if (o.kind == OP_HEAD2 || o.kind == OP_HEADBF) c.head2_op = (int)k;
        if (o.out >= 0 && c.tensors[o.out].def < 0) c.tensors[o.out].def = (int)k;
        if (o.out2 >= 0 && c.tensors[o.out2].def < 0) c.tensors[o.out2].def = (int)k;
        auto use = [&](int t) { if (t >= 0) c.tensors[t].last = std::max(c.tensors[t].last, (int)k); };
        use(o.in); use(o.res);
        for (int t = 0; t < 4; ++t) use(o.terms[t]);
    }
    // the multi-head groups refer to op indices too
    for (Multi& m : c.multis) m.n = 0;
    for (size_t k = 0; k < c.ops.size(); ++k)
        if (c.ops[k].multi >= 0) { Multi& m = c.multis[c.ops[k].multi]; m.op[c.ops[k].mpos] = (int)k; m.n = std::max(m.n, c.ops[k].mpos + 1); }
}

// Post-pass: lanes and waves.  Lane 0 is the caller's stream (the trunk), lanes 1..3 are side streams.  A launch unit (one
// op, or the consecutive members of a job / multi-head group) is placed by what it depends on among the not yet joined
// launches of the current wave — earlier writers of what it reads, earlier readers and writers of what it writes:
//   lane 0 only, incl. its tail   -> lane 0: it continues the trunk;
//   lane 0 only, not the tail     -> it forks onto the least loaded side lane behind the event of its latest lane-0
//                                    dependency (or the wave's entry event): what lane 0 has queued since runs beside it;
//   one side lane, not the trunk tail -> that side lane (behind the event of its latest lane-0 dependency, if newer);
//   one side lane + the trunk tail, or two and more side lanes -> lane 0, which first waits for those side lanes (join).
// A join that covers every side lane with work in flight ends the wave: all earlier launches are complete when the joining
// unit starts.  plan_shape() keeps a tensor alive to the end of the wave of its last reader, so recycled scratch adds no
// dependency inside a wave, and the schedule — true dependencies only — does not depend on the shape.
// Side lanes only ever wait on events of lane 0, and lane 0 on theirs: ROCm 7.x overflows its stack in
// hipStreamEndCapture when two non-origin streams of one capture have waited on each other (found with
// tools/ubench/segv_bt.c); fork/join through the origin stream captures fine (tools/ubench/graph_branches.hip).
void schedule_waves(esahrnet_ctx& c) {
    const size_t nops = c.ops.size();
    for (Op& o : c.ops) { o.lane = 0; o.wave = 0; o.wait0 = -1; o.wait_entry = false; o.record = false; o.join = 0; }
    c.nwaves = 1;
    if (c.opt.nlanes > 1) {
        std::vector<std::vector<int>> readers(c.tensors.size()), writers(c.tensors.size());
        std::vector<int> unit_end(nops, 0);       // op -> last op of its launch unit
        int wave = 0, wave_start = 0, tail0 = -1;
        int load[4], waited0[4], tail[4], joined_tail[4], joined_op[4];
        bool active[4];
        auto reset = [&]() {
            for (int l = 0; l < 4; ++l) { load[l] = 0; waited0[l] = -1; tail[l] = -1; joined_tail[l] = -1; joined_op[l] = -1; active[l] = false; }
        };
        reset();
        for (size_t k = 0; k < nops;) {
            size_t e = k + 1;
            while (e < nops && ((c.ops[k].job >= 0 && c.ops[e].job == c.ops[k].job) ||
                                (c.ops[k].multi >= 0 && c.ops[e].multi == c.ops[k].multi))) ++e;
            unsigned side = 0;
            int zmax = -1;
            auto dep = [&](int d) {
                if (d < wave_start || d >= (int)k) return;
                const int l = c.ops[d].lane;
                if (l == 0) zmax = std::max(zmax, unit_end[d]);
                else if (d <= joined_tail[l]) zmax = std::max(zmax, joined_op[l]);      // already joined into the trunk
                else side |= 1u << l;
            };
            for (size_t m = k; m < e; ++m) {
                const Op& o = c.ops[m];
                for (int t : {o.in, o.res, o.terms[0], o.terms[1], o.terms[2], o.terms[3]})
                    if (t >= 0) for (int w : writers[t]) dep(w);
                if (o.out >= 0) {
                    for (int r : readers[o.out]) dep(r);
                    for (int w : writers[o.out]) dep(w);
                }
            }
            Op& lead = c.ops[k];
            int lane = 0;
            const int nside = __builtin_popcount(side);
            if (nside >= 2 || (nside == 1 && zmax == tail0)) {
                lead.join = side;
                bool all = true;
                for (int l = 1; l < 4; ++l) if (active[l] && !(side >> l & 1)) all = false;
                if (all) {
                    ++wave; wave_start = (int)k; tail0 = -1;
                    reset();
                } else {
                    for (int l = 1; l < 4; ++l)
                        if (side >> l & 1) { active[l] = false; joined_tail[l] = tail[l]; joined_op[l] = (int)e - 1; }
                }
            } else if (nside == 1) {
                lane = __builtin_ctz(side);
            } else if (zmax != tail0) {
                lane = 1;
                for (int l = 2; l < 4; ++l) if (load[l] < load[lane]) lane = l;
            }
            if (lane) {
                if (zmax > waited0[lane]) { lead.wait0 = zmax; c.ops[zmax].record = true; waited0[lane] = zmax; }
                else if (waited0[lane] < 0 && tail[lane] < 0) lead.wait_entry = true;
                active[lane] = true;
            }
            ++load[lane];
            for (size_t m = k; m < e; ++m) {
                Op& o = c.ops[m];
                o.lane = lane; o.wave = wave;
                unit_end[m] = (int)e - 1;
                for (int t : {o.in, o.res, o.terms[0], o.terms[1], o.terms[2], o.terms[3]}) if (t >= 0) readers[t].push_back((int)m);
                if (o.out >= 0) writers[o.out].push_back((int)m);
            }
            tail[lane] = (int)e - 1;
            if (!lane) tail0 = (int)e - 1;
            k = e;
        }
        c.nwaves = wave + 1;
    }
    c.wave_last.assign(c.nwaves, 0);
    c.wave_mask.assign(c.nwaves, 0);
    for (size_t k = 0; k < nops; ++k) {
        c.wave_last[c.ops[k].wave] = (int)k;
        c.wave_mask[c.ops[k].wave] |= (unsigned char)(1u << c.ops[k].lane);
    }
}

int build_plan_ops(esahrnet_ctx& c) {
    const esahrnet_cfg& g = c.cfg;
    Builder B(c);
    const int sw = g.stem_width;
    // ---- stem (seg_hrnet.py:265-270, 426-431) ----
    c.spec_stem = B.spec("conv1", "bn1", g.cin, sw, 3, 1, 0, false, true);
    const int spec_conv2 = B.spec("conv2", "bn2", sw, sw, 3, 2, 1, false, true);
    int x;
    int stem_raw = -1;
    if (g.variant == 1) {   // seg_hrnet3.py:473-475: x0 = conv1(x0) is kept (pre-BN) for the CBAM skip: conv1 a second time
        Op o; o.kind = OP_STEMRAW; o.out = B.tensor(sw, 0, "stem_raw"); stem_raw = o.out;
        o.aux[0] = B.aux("conv1.weight", sw, g.cin, 3, 3); B.push(o);
    }
    if (c.opt.stem != STEM_SEPARATE) {  // conv1 + bn1 + ReLU recomputed per tile inside the conv2 kernel (stem_fused.hip / conv_x6.hip)
        DevConv d;
        d.spec = spec_conv2; d.c0 = 0; d.c1 = sw; d.use_bias = true;
        d.cinp = pad32(sw); d.coutp = pad32(sw);
        c.dconvs.push_back(d);
        Op o; o.kind = OP_STEMF; o.dconv = (int)c.dconvs.size() - 1; o.out = B.tensor(sw, 1, "stem2");
        B.push(o);
        x = o.out;
    } else {                // conv1 + bn1 + ReLU on the stem kernel, conv2 on the stream kernel
        Op o; o.kind = OP_STEM; o.out = B.tensor(sw, 0, "stem1");
        B.push(o);
        x = B.conv(spec_conv2, o.out, -1, true, "stem2");
    }
    // ---- layer1 (:277, :432) ----
    int cin = sw;
    const int nb1 = g.blocks[0][0];
    for (int k = 0; k < nb1; ++k) {
        x = B.basic_block("layer1." + std::to_string(k), x, cin, g.widths[0], 1, k == nb1 - 1 ? "layer1" : "");
        cin = g.widths[0];
    }
    std::vector<int> ys{x};
    std::vector<int> pre{g.widths[0]};
    for (int s = 2; s <= 4; ++s) {
        int nb = 0;
        while (nb < ESAHRNET_MAX_BRANCHES && g.blocks[s - 1][nb] > 0) ++nb;
        if (nb < (int)pre.size() || nb > (int)pre.size() + 1)
            return set_error("stage %d: %d branches after %zu (must grow by at most one)", s, nb, pre.size());
        std::vector<int> cur(g.widths, g.widths + nb);
        const std::string t = "transition" + std::to_string(s - 1);
        // ---- transition (:343-377, wiring :434-457: new branch from ys.back()) ----
        std::vector<int> xs;
        for (int i = 0; i < nb; ++i) {
            if (i < (int)pre.size()) {
                if (pre[i] != cur[i]) {
                    const std::string q = t + "." + std::to_string(i);
                    xs.push_back(B.conv(B.spec(q + ".0", q + ".1", pre[i], cur[i], 3, 1, 1 + i, false, true), ys[i], -1, true));
                } else {
                    xs.push_back(ys[i]);
                }
            } else {
                int tt = ys.back();
                const int nconv = i + 1 - (int)pre.size();
                for (int j = 0; j < nconv; ++j) {
                    const std::string q = t + "." + std::to_string(i) + "." + std::to_string(j);
                    const int co = j == nconv - 1 ? cur[i] : pre.back();
                    tt = B.conv(B.spec(q + ".0", q + ".1", pre.back(), co, 3, 2, (int)pre.size() + j + 1, false, true), tt, -1, true);
                }
                xs.push_back(tt);
            }
        }
        // ---- HighResolutionModule x NUM_MODULES (:105-249) ----
        for (int m = 0; m < g.modules[s - 1]; ++m) {
            const std::string p = "stage" + std::to_string(s) + "." + std::to_string(m);
            for (int b = 0; b < nb; ++b) {
                for (int k = 0; k < g.blocks[s - 1][b]; ++k) {
                    // conv1 / conv2 of block k take keys 2k / 2k + 1 (seg_hrnet3: 6k .. 6k + 5 with the block's CBAM launches)
                    B.jkey = (((s << 4) | m) << 8) | ((g.variant == 1 ? 6 : 2) * k);
                    xs[b] = B.basic_block(p + ".branches." + std::to_string(b) + "." + std::to_string(k),
                                          xs[b], cur[b], cur[b], 1 + b, "");
                    B.jkey = -1;
                }
            }
            // fuse layers (:176-220, :232-247).  Emitted family by family, not output branch by output branch, so that
            // independent launches of one kernel family stand next to each other (group_jobs / group_multihead merge them):
            // all 1x1 fuse-up convolutions, then the stride-2 fuse-down chains link by link, then the sums.
            std::vector<std::vector<int>> terms(nb, std::vector<int>(nb, -1));
            const int modkey = ((s << 4) | m) << 8;
            for (int i = 0; i < nb; ++i) {
                terms[i][i] = xs[i];
                for (int j = i + 1; j < nb; ++j) {      // 1x1 + BN on the low-res grid; up-sampled inside fuse
                    const std::string q = p + ".fuse_layers." + std::to_string(i) + "." + std::to_string(j);
                    B.jkey2 = modkey | 100;             // all fuse-up 1x1 convolutions of the module are independent (before the chains)
                    terms[i][j] = B.conv(B.spec(q + ".0", q + ".1", cur[j], cur[i], 1, 1, 1 + j, false, false), xs[j], -1, false);
                    B.jkey2 = -1;
                }
            }
            for (int k = 0; k + 1 < nb; ++k)            // link k of every chain of 3x3 s2 (:198-217) that has one
                for (int i = k + 1; i < nb; ++i)
                    for (int j = 0; j + k < i; ++j) {
                        const bool last = k == i - j - 1;
                        const std::string qq = p + ".fuse_layers." + std::to_string(i) + "." + std::to_string(j) + "." + std::to_string(k);
                        const int sp_ = B.spec(qq + ".0", qq + ".1", cur[j], last ? cur[i] : cur[j], 3, 2, 1 + j + k + 1, false, !last);
                        B.jkey2 = modkey | (128 + k);
                        terms[i][j] = B.conv(sp_, k == 0 ? xs[j] : terms[i][j], -1, !last);
                        B.jkey2 = -1;
                    }
            std::vector<int> outs;
            for (int i = 0; i < nb; ++i) {
                const bool final_module = m == g.modules[s - 1] - 1;
                outs.push_back(B.fuse(terms[i], cur[i], 1 + i, true,
                                      final_module ? "stage" + std::to_string(s) + "." + std::to_string(i) : "",
                                      p + ".fuse." + std::to_string(i)));
            }
            xs = outs;
        }
        ys = xs;
        pre = cur;
    }
    // ---- head (:313-340, :461-469) ----
    int tot = 0;
    for (int v : pre) tot += v;
    const int K = g.num_keypoints;
    if (g.variant == 1) {
        // seg_hrnet3.py:363-383, 506-520: cat of the up-sampled branches (materialised: last_layer[0] is a
        // 3x3 conv here), 3x3 480->480, 1x1 480->K, up x2 (align_corners=True), cat with CBAM(stem skip),
        // 3x3 (K+64)->K.  The second concat is laid out [skip | heat-maps] so that both slices start on
        // an 8-channel group; output_layer's input channels are permuted accordingly when packed.
        // bf16 mode: the direct head below (no gather), and the output layer leaves its heat-maps in f32 (out_f32: the
        // stream kernel's f32 epilogue), as variant 0's bf16 output layer does.
        const int l0 = B.spec("last_layer.0", "last_layer.1", tot, tot, 3, 1, 1, true, true);
        const int l3 = B.spec("last_layer.3", "last_layer.4", tot, K, 1, 1, 1, true, true);
        c.spec_final = B.spec("output_layer.0", "", K + sw, K, 3, 1, 0, true, false);
        int h0, wide_h0 = 0;
        if (ys.size() == 4 && !c.h16() && !c.opt.head3_direct) {
            // last_layer[0] by linearity (head_gather.hip): branches 2, 3 as nine 1x1 products on their own grids + a gather,
            // branch 0 and the up-sampled branch 1 as a direct 3x3 that takes the gather's result as its residual
            const int cd = pre[0] + pre[1];
            const int cat = B.tensor(cd, 1, "head_cat");
            int off = 0;
            for (int b = 0; b < 2; ++b) {
                Op o; o.kind = OP_RESAMPLE; o.in = ys[b]; o.out = cat; o.c0 = off; o.nchan = pre[b]; o.align = 0;
                B.push(o);
                off += pre[b];
            }
            if (pad32(cd) > ((cd + 7) & ~7)) {
                Op o; o.kind = OP_ZERO; o.out = cat; o.terms[0] = cat; o.c0 = (cd + 7) & ~7; o.nchan = pad32(cd) - ((cd + 7) & ~7);
                B.push(o);
            }
            int z[2];
            for (int b = 2; b < 4; ++b) {
                const int zs = B.taps_spec(l0, off, off + pre[b], 1 + b);
                z[b - 2] = B.conv(zs, ys[b], -1, false, "", 0, -1, false, true);      // plain f32: the gather needs no join
                off += pre[b];
            }
            Op gop; gop.kind = OP_GATHER; gop.in = z[0]; gop.nterms = 1; gop.terms[0] = z[1];
            gop.out = B.tensor(tot, 1, "head_gather");
            B.push(gop);
            h0 = B.conv(l0, cat, gop.out, true, "head0", 0, cd);
            // 64-cout workgroup slices for the direct convolution: the stream kernel stages an input tile once per 64 instead of
            // once per 32 couts (480 = 7.5 x 64: the output, its residual and the reader's input are padded to 512 channels,
            // the padding is exact zeros end to end: zero weights, zero bias, zero residual)
            if (pad64(tot) != pad32(tot) && !c.opt.head3_cout32) {
                const int cp = pad64(tot);
                c.tensors[gop.out].Cp = cp;
                c.tensors[h0].Cp = cp;
                c.dconvs[c.ops.back().dconv].coutp = cp;
                wide_h0 = cp;
            }
        } else {
            const int cat = B.tensor(tot, 1, "head_cat");
            int off = 0;
            for (size_t b = 0; b < ys.size(); ++b) {
                Op o; o.kind = OP_RESAMPLE; o.in = ys[b]; o.out = cat; o.c0 = off; o.nchan = pre[b]; o.align = 0;
                B.push(o);
                off += pre[b];
            }
            if (c.padc(tot) > ((tot + 7) & ~7)) {
                Op o; o.kind = OP_ZERO; o.out = cat; o.terms[0] = cat; o.c0 = (tot + 7) & ~7; o.nchan = c.padc(tot) - ((tot + 7) & ~7);
                B.push(o);
            }
            h0 = B.conv(l0, cat, -1, true, "head0");
        }
        const int h3 = B.conv(l3, h0, -1, true, "head3");
        if (wide_h0) c.dconvs[c.ops.back().dconv].cinp = wide_h0;
        const int cat2 = B.tensor(sw + K, 0, "head_cat2");
        const int first_cbam_op = (int)c.ops.size();
        B.cbam("", stem_raw, sw, -1, false, cat2, 0);
        // the pooling over the raw stem tensor rides in the kernel that writes it (stem.hip: launch_stem_pool): that op also
        // owns the partials, sized for the slabs that kernel makes (one per row piece) instead of pool_partial's 64
        if (c.ops[first_cbam_op].kind == OP_POOL && c.ops[first_cbam_op].in == stem_raw && !c.opt.stem_pool_separate)
            for (Op& so : c.ops)
                if (so.kind == OP_STEMRAW) {
                    const int partial = c.ops[first_cbam_op].out;
                    so.out2 = partial;
                    c.tensors[partial].flat = esa::STEM_POOL_SLABS_MAX * c.tensors[stem_raw].Cp * 2;
                    c.stemraw_partial = partial;
                }
        { Op o; o.kind = OP_RESAMPLE; o.in = h3; o.out = cat2; o.terms[0] = cat2; o.c0 = sw; o.nchan = K; o.align = 1; B.push(o); }
        if (c.padc(sw + K) > sw + ((K + 7) & ~7)) {
            Op o; o.kind = OP_ZERO; o.out = cat2; o.terms[0] = cat2; o.c0 = sw + ((K + 7) & ~7); o.nchan = c.padc(sw + K) - o.c0;
            B.push(o);
        }
        const int oc = B.conv(c.spec_final, cat2, -1, false, "out_sb", 0, -1, true, c.h16());
        std::vector<int>& perm = c.dconvs[c.ops.back().dconv].perm;     // packed ci -> reference ci
        for (int i = 0; i < sw; ++i) perm.push_back(K + i);              // skip channels come second in the reference
        for (int i = 0; i < K; ++i) perm.push_back(i);
        { Op o; o.kind = OP_TONCHW; o.in = oc; B.push(o); }
        return 0;
    }
    const int l0 = B.spec("last_layer.0", "last_layer.1", tot, tot, 1, 1, 1, true, true);
    const int l3 = B.spec("last_layer.3", "last_layer.4", tot, K, 1, 1, 1, true, true);
    c.spec_final = B.spec("output_layer.0", "", K + g.cin, K, 3, 1, 0, true, false);
    int h3;
    if (c.opt.head == HEAD_SB) {
        // t_b = W_b x_b on branch b's grid (f32 NHWC), b = 1..3; W_0, bias, ReLU, last_layer[3..5]
        // and the up-sampling of the t_b all happen inside head_fused.hip
        c.spec_l0 = l0; c.spec_l3 = l3; c.head_c0 = pre[0];
        // Two alternatives, chosen per input shape (plan_shape): alt 2 = head_t.hip + head_fused2.hip
        // (interpolation on the matrix cores, t_1 never materialised) when its geometry checks pass,
        // alt 1 = f32 NHWC terms + head_fused.hip otherwise.  Both read the same packed W_b slices.
        Op o; o.kind = OP_HEAD; o.in = ys[0]; o.nterms = 3; o.alt = c.opt.head2 ? 1 : 0;
        int off = pre[0];
        int dslice[4] = {-1, -1, -1, -1};
        for (int b = 1; b < 4; ++b) {
            const int save = c.specs[l0].level;
            c.specs[l0].level = 1 + b;
            o.terms[b - 1] = B.conv(l0, ys[b], -1, false, "", off, off + pre[b], false, true);
            c.ops.back().alt = o.alt;
            c.tensors[o.terms[b - 1]].alt = o.alt;
            dslice[b] = c.ops.back().dconv;
            c.specs[l0].level = save;
            off += pre[b];
        }
        o.out = B.tensor(K, 1, "head3");
        c.tensors[o.out].Cp = (K + 15) & ~15;     // read only by head.hip: 16-channel pitch halves its traffic for K <= 16
        const int idx = (int)c.ops.size();
        c.tensors[o.out].def = idx;
        B.use(o.in, idx);
        for (int i = 0; i < 3; ++i) B.use(o.terms[i], idx);
        c.ops.push_back(o);
        h3 = o.out;
        if (c.opt.head2) {
            int tt[4] = {-1, -1, -1, -1};
            for (int b = 2; b < 4; ++b) {
                Op t; t.kind = OP_HEADT; t.in = ys[b]; t.dconv = dslice[b]; t.alt = 2;
                t.out = B.tensor(tot, 1 + b);
                c.tensors[t.out].tlayout = true;
                c.tensors[t.out].alt = 2;
                B.push(t);
                tt[b] = t.out;
            }
            Op q; q.kind = OP_HEAD2; q.in = ys[0]; q.nterms = 3; q.alt = 2; q.dconv = dslice[1];
            q.terms[0] = ys[1]; q.terms[1] = tt[2]; q.terms[2] = tt[3];
            q.out = h3;
            c.head2_op = B.push(q);
        }
    } else {
        // bf16 mode: the slices t_1..t_3 are shared by two alternatives, chosen per input shape (plan_shape):
        // alt 2 = head_fused_bf.hip (W0, interpolation, ReLU, last_layer[3] in one kernel) where its source-region
        // geometry holds, alt 1 = slice 0 + fuse + 1x1 (the 720-channel tensors materialised) otherwise
        // (fp32-grade mode: the same arrangement with head_x6.hip; f32 NHWC slices, ESAHRNET_X6_UNFUSED_HEAD=1 keeps alt 1)
        const bool bf_head = c.opt.head == HEAD_BF || c.opt.head == HEAD_X6;
        std::vector<int> hterms(ys.size(), -1);
        int off = 0;
        std::vector<int> offs;
        for (size_t b = 0; b < ys.size(); ++b) { offs.push_back(off); off += pre[b]; }
        for (size_t b = bf_head ? 1 : 0; b < ys.size(); ++b) {
            // the slice runs at branch b's own resolution: fix the output level of the slice conv
            const int save = c.specs[l0].level;
            c.specs[l0].level = 1 + (int)b;
            hterms[b] = B.conv(l0, ys[b], -1, false, "", offs[b], offs[b] + pre[b], b == 0);
            c.specs[l0].level = save;
        }
        int h3b = -1;
        if (bf_head) {
            const int first_alt1 = (int)c.ops.size();
            const int save = c.specs[l0].level;
            hterms[0] = B.conv(l0, ys[0], -1, false, "", 0, pre[0], true);
            c.specs[l0].level = save;
            c.spec_l0 = l0; c.spec_l3 = l3; c.head_c0 = pre[0];
            Op q; q.kind = OP_HEADBF; q.in = ys[0]; q.nterms = 3; q.alt = 2;
            for (int b = 1; b < 4; ++b) q.terms[b - 1] = hterms[b];
            q.out = B.tensor(K, 1, "head3_fused");
            c.tensors[q.out].Cp = K <= 16 ? 16 : 32;      // read only by the output-layer kernel
            c.tensors[q.out].alt = 2;
            h3b = q.out;
            // alternative 1 first (its ops and tensors carry alt = 1), then the fused op
            const int h0 = B.fuse(hterms, tot, 1, true, "head0");
            h3 = B.conv(l3, h0, -1, true, "head3");
            for (int k = first_alt1; k < (int)c.ops.size(); ++k) {
                c.ops[k].alt = 1;
                if (c.ops[k].out >= 0) c.tensors[c.ops[k].out].alt = 1;
            }
            c.head2_op = B.push(q);
        } else {
            const int h0 = B.fuse(hterms, tot, 1, true, "head0");
            h3 = B.conv(l3, h0, -1, true, "head3");
        }
        if (h3b >= 0) {
            Op o; o.kind = OP_FINAL; o.in = h3b; o.alt = 2;
            B.push(o);
            Op o1; o1.kind = OP_FINAL; o1.in = h3; o1.alt = 1;
            B.push(o1);
            return 0;
        }
    }
    {
        Op o; o.kind = OP_FINAL; o.in = h3;
        B.use(h3, (int)c.ops.size());
        c.ops.push_back(o);
    }
    return 0;
}

}  // namespace

int build_plan(esahrnet_ctx& c) {
    if (build_plan_ops(c)) return 1;
    group_multihead(c);
    group_jobs(c);
    schedule_waves(c);
    return 0;
}

// ---- fp16 scale groups ------------------------------------------------------------------------------------
// With BatchNorm folded, seg_hrnet / seg_hrnet2 is convolution, bias, ReLU, sums and bilinear interpolation, all of which
// commute exactly with a power of two: tensor T may be stored as T * 2^-e if the next convolution's weights take 2^(e_in -
// e_out) and its bias 2^-e_out.  Tensors that reach each other WITHOUT convolution weights in between must share e: a
// residual and the sum it enters, the terms of a fuse sum and its result, the slices of last_layer[0] with the h0 the fused
// head forms from them in registers, the head3 of either head alternative (one output layer reads both).  Read off the op
// list, so every stage table gets its own groups.  Groups are numbered by their first tensor in plan order.
int build_scale_groups(esahrnet_ctx& c) {
    c.tgroup.assign(c.tensors.size(), -1);
    c.gnames.clear();
    c.exps.clear();
    if (c.cfg.variant != 0 || !c.h16()) return 0;
    std::vector<int> parent(c.tensors.size());
    for (size_t i = 0; i < parent.size(); ++i) parent[i] = (int)i;
    auto find = [&](int a) { while (parent[a] != a) a = parent[a] = parent[parent[a]]; return a; };
    auto join = [&](int a, int b) {
        if (a < 0 || b < 0) return;
        a = find(a); b = find(b);
        if (a != b) parent[std::max(a, b)] = std::min(a, b);      // the root is the group's first tensor
    };
    int final_in = -1;
    for (const Op& o : c.ops) {
        switch (o.kind) {
            case OP_STEM: break;
            case OP_CONV: join(o.out, o.res); break;
            case OP_FUSE: for (int i = 0; i < o.nterms; ++i) join(o.out, o.terms[i]); break;
            case OP_HEADBF: for (int i = 1; i < o.nterms; ++i) join(o.terms[0], o.terms[i]); break;
            case OP_FINAL: join(final_in, o.in); final_in = o.in; break;
            default: return set_error("scale groups: the plan holds an op (kind %d) the 16-bit formats of variant 0 do not have", (int)o.kind);
        }
    }
    std::vector<int> gid(c.tensors.size(), -1);
    for (size_t t = 0; t < c.tensors.size(); ++t) {
        if (c.tensors[t].flat || c.tensors[t].f32 || c.tensors[t].def < 0) continue;
        const int r = find((int)t);
        if (gid[r] < 0) { gid[r] = (int)c.gnames.size(); c.gnames.push_back(""); }
        c.tgroup[t] = gid[r];
    }
    // names: the branch stream a "stageS.I" tap belongs to, else a tap of the group (stem1, stem2, head0, head3), else the
    // convolution that writes the group's first tensor
    for (size_t t = 0; t < c.tensors.size(); ++t) {
        const int g = c.tgroup[t];
        if (g < 0) continue;
        const std::string& tap = c.tensors[t].tap;
        int s = 0, i = 0;
        char tail = 0;
        if (sscanf(tap.c_str(), "stage%d.%d%c", &s, &i, &tail) == 2) c.gnames[g] = "stream" + std::to_string(i);
        else if (c.gnames[g].empty() && !tap.empty() && tap.compare(0, 5, "conv:") != 0 && tap != "layer1" && tap != "head3_fused") c.gnames[g] = tap;
    }
    for (size_t t = 0; t < c.tensors.size(); ++t) {
        const int g = c.tgroup[t];
        if (g < 0 || !c.gnames[g].empty()) continue;
        const Op& o = c.ops[c.tensors[t].def];
        c.gnames[g] = o.kind == OP_CONV ? c.specs[c.dconvs[o.dconv].spec].name : "tensor" + std::to_string(t);
    }
    c.exps.assign(c.gnames.size(), 0);
    return 0;
}

// Where convolution `index` (a host spec) sits among the groups: the group its output is stored in (-1: none, the f32 heat-maps)
// and the group of each range of its input channels (-1: the f32 crop), ranges in channel order.
int scale_conv_info(const esahrnet_ctx& c, int index, int* out_group, std::vector<ScaleRange>& ranges) {
    ranges.clear();
    const ConvSpec& s = c.specs[index];
    if (c.gnames.empty()) return set_error("scale groups: this handle has none (variant 0 with precision 1 or 3 only)");
    int og = -2;
    auto add = [&](int c0, int c1, int in_group, int out) -> int {
        if (og != -2 && og != out) return set_error("scale groups: the outputs of '%s' lie in two groups", s.name.c_str());
        og = out;
        for (const ScaleRange& r : ranges)
            if (r.c0 == c0) return r.c1 == c1 && r.group == in_group ? 0 : set_error("scale groups: input slices of '%s' disagree", s.name.c_str());
        ranges.push_back({c0, c1, in_group});
        return 0;
    };
    for (const Op& o : c.ops) {
        if (o.kind == OP_STEM && index == c.spec_stem) { if (add(0, s.cin, -1, c.tgroup[o.out])) return 1; }
        else if (o.kind == OP_FINAL && index == c.spec_final) {
            const int K = c.cfg.num_keypoints;
            if (add(0, K, c.tgroup[o.in], -1) || add(K, s.cin, -1, -1)) return 1;
        } else if (o.kind == OP_CONV && c.dconvs[o.dconv].spec == index) {
            const DevConv& d = c.dconvs[o.dconv];
            if (add(d.c0, d.c1, c.tgroup[o.in], c.tgroup[o.out])) return 1;
        } else if (o.kind == OP_HEADBF && index == c.spec_l0) {
            if (add(0, c.head_c0, c.tgroup[o.in], c.tgroup[o.terms[0]])) return 1;
        } else if (o.kind == OP_HEADBF && index == c.spec_l3) {
            if (add(0, s.cin, c.tgroup[o.terms[0]], c.tgroup[o.out])) return 1;
        }
    }
    std::sort(ranges.begin(), ranges.end(), [](const ScaleRange& a, const ScaleRange& b) { return a.c0 < b.c0; });
    int at = 0;
    for (const ScaleRange& r : ranges) { if (r.c0 != at) break; at = r.c1; }
    if (og == -2 || at != s.cin) return set_error("scale groups: the plan does not cover the input channels of '%s'", s.name.c_str());
    *out_group = og;
    return 0;
}

// Convolution `index` as esahrnet_commit packs it: the host's folded weights with 2^(e_in - e_out) on every range of input
// channels and 2^-e_out on the bias — ldexpf, exact unless the result leaves f32's normal range.  shift_at (optional): the
// exponent each input channel's weights were given.
int scaled_conv(const esahrnet_ctx& c, int index, std::vector<float>& w, std::vector<float>& b, std::vector<int>* shift_at) {
    const ConvSpec& s = c.specs[index];
    w = s.w; b = s.b;
    if (shift_at) shift_at->assign(s.cin, 0);
    if (!c.scaled()) return 0;
    int og = -1;
    std::vector<ScaleRange> ranges;
    if (scale_conv_info(c, index, &og, ranges)) return 1;
    const int taps = s.k * s.k, eo = c.gexp(og);
    for (const ScaleRange& r : ranges) {
        const int sh = c.gexp(r.group) - eo;
        for (int ci = r.c0; ci < r.c1; ++ci) {
            if (shift_at) (*shift_at)[ci] = sh;
            if (!sh) continue;
            for (int co = 0; co < s.cout; ++co)
                for (int t = 0; t < taps; ++t) {
                    float& v = w[((size_t)co * s.cin + ci) * taps + t];
                    v = ldexpf(v, sh);
                }
        }
    }
    if (eo) for (float& v : b) v = ldexpf(v, -eo);
    for (float v : w)
        if (!std::isfinite(v)) return set_error("commit: a weight of '%s' is not finite in f32 under its scale shift", s.name.c_str());
    for (float v : b)
        if (!std::isfinite(v)) return set_error("commit: a bias of '%s' is not finite in f32 under its scale shift 2^%d", s.name.c_str(), -eo);
    return 0;
}

}  // namespace esa
