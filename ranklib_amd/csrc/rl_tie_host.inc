// rl_tie_host.inc -- the host side of the lazy Java-order tie-break: the stages of one resolution, in the order resolve_ties (at the end of this
// file) calls them.  Included by rl_trainer.hip behind `struct rl_trainer`, which the stages dereference (the kernels they launch are in
// rl_tie.inc, ahead of the struct), and in front of rl_round.inc, whose growth stages call resolve_ties.
//
// The device stalled the tree on nodes whose exactly tied best split the Java's rounding noise decides.  The stream is idle when a resolution
// starts (the caller synchronised it).  It reads the node records, lays out the derivation chains -- a node the Java accumulates (root / left
// child) is summed from its members; a right child is parent - left sibling, recursively -- and runs the kernels that put the Java's choice
// into the node records and resume the growth bookkeeping:
//
//   tie_read_tree      TreeState and node records through the pinned buffer; the nodes to resolve
//   tie_plan_chains    host only: chain nodes, path predicates, the nodes to verify, the flattened chains; fixed_bytes
//   tie_stage1         device: tied candidates (k_tie_cand), verification of deferred cuts (k_tie_verify), member lists; reads need[] and the
//                      local member counts back unless the walk was chosen up front
//   tie_plan_pairs, tie_read_bin_counts, tie_plan_spec     the needed (chain node, feature) pairs; their cumulative bin counts (a device read);
//                      host only again: the contiguous chains with their windows and chunks; spec_bytes
//   tie_reserve_spec   the memory decision: grows the arena and, as it moves, runs tie_stage1 again
//   tie_eval_walk | tie_eval_spec     the per-bin Java-order sums: the literal walk, or the speculative chains (tie_gather_local |
//                      tie_gather_sharded put the members' values into global member order first)
//   tie_commit         k_tie_prefix, k_tie_eval, k_tie_finish, the verdict of k_tie_verify, the counters
//
// What lives how long.  The trainer keeps the scratch arena (tie_buf: it only ever grows, and MOVES when it does), the pinned buffer (tie_pin:
// the same) and the host blob across resolutions.  Within one resolution the host plans (TiePlan, TieSpecPlan) are plain values that no device
// call invalidates.  Every device pointer into the arena lives in a TieStage1, which tie_stage1 fills completely from the arena as it then
// stands: whoever moves the arena runs tie_stage1 again on the same TieStage1, and nothing else holds such a pointer across a stage boundary
// (SpArgs and the gathers' pieces are taken and used up inside tie_eval_spec).  The pinned buffer: a stage asks tie_pin_reserve for what it
// reads and takes t->tie_pin afterwards; every use is copy, synchronise, memcpy, so nothing in flight reads the buffer when it moves.
//
// Sharded runs (tie_ranks(t) > 1): the flags come from all-reduced histograms, so every rank resolves the same nodes and plans the same chains;
// only the member counts (lcnt) and with them spec_bytes differ.  Every rank issues the same collectives in the same order: the OP_MAX
// all-reduce of the out-of-memory flag in tie_reserve_spec on every resolution, whether or not the rank grows; the all-gather of the counts and
// the one or two all-to-alls of tie_gather_sharded; the OP_MAX all-reduce of the verification flag in tie_commit when nodes were verified.  A
// sharded resolution never takes the walk (it sums this rank's documents only), so no rank can leave the others waiting in a collective.

namespace rl {

// ---- what the trainer keeps: the scratch arena, the pinned buffer, the host blob ---------------------------------------
struct TieArena {
    char *base = nullptr; size_t cap = 0, used = 0;
    template <class T> T *take(size_t n) { used = (used + 255) & ~(size_t)255; T *p = (T *)(base + used); used += n * sizeof(T); return p; }
};
static int tie_arena_reserve(rl_trainer *t, size_t bytes)
{
    if (bytes <= t->tie_cap) return RL_OK;
    if (t->tie_buf) { (void)hipFree(t->tie_buf); t->tie_buf = nullptr; t->tie_cap = 0; }
    const size_t want = bytes + bytes / 4 + (1 << 20);
    if (hipMalloc(&t->tie_buf, want) != hipSuccess) { (void)hipGetLastError(); t->tie_buf = nullptr; return RL_ERR_HIP; }
    t->tie_cap = want;
    return RL_OK;
}
// small reads come back through one pinned buffer (a pageable copy costs tens of microseconds each).  It grows with what a resolution needs:
// a batch of deferred nodes of a tree with hundreds of leaves, or of wide data with many tied features, is not a reason to stop training
static int tie_pin_reserve(rl_trainer *t, size_t bytes)
{
    if (t->tie_pin_cap >= bytes) return RL_OK;
    if (t->tie_pin) (void)hipHostFree(t->tie_pin);
    t->tie_pin = nullptr; t->tie_pin_cap = 0;
    const size_t want = bytes + bytes / 4;
    if (hipHostMalloc(&t->tie_pin, want, hipHostMallocDefault) != hipSuccess) { (void)hipGetLastError(); return fail(RL_ERR_HIP, "tie-break: no pinned host memory"); }
    t->tie_pin_cap = want;
    return RL_OK;
}
// the small host tables of a stage travel as ONE copy: put() appends a table at a 16-byte boundary and returns its offset
struct TieBlob {
    std::vector<char> &b;
    explicit TieBlob(rl_trainer *t) : b(t->tie_blob) { b.clear(); }
    size_t put(const void *src, size_t bytes) { const size_t o = (b.size() + 15) & ~(size_t)15; b.resize(o + bytes); if (bytes) memcpy(b.data() + o, src, bytes); return o; }
    int upload(TieArena &ar, hipStream_t s, char **d_blob) const
    {
        *d_blob = ar.take<char>(b.size() + 16);
        RL_HIP(hipMemcpyAsync(*d_blob, b.data(), b.size(), hipMemcpyHostToDevice, s));
        return RL_OK;
    }
};
static int tie_ranks(const rl_trainer *t) { return (t->dist && t->n_ranks > 1) ? t->n_ranks : 1; }      // > 1: sharded, the members of a chain node are spread over the ranks

// ---- the tree as the device left it, and the nodes to resolve ----------------------------------------------------------
// deferred = false: the nodes the tree is stalled on (TreeState::stall_node); deferred = true: the committed nodes flagged 0x40
static int tie_read_tree(rl_trainer *t, bool deferred, std::vector<NodeRec> &nodes, std::vector<int> &todo)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    { int rcp = tie_pin_reserve(t, sizeof(TreeState) + (size_t)(c.NC + 2) * sizeof(NodeRec) + (size_t)kTieMaxChain * c.F * 4 + ((size_t)1 << 20)); if (rcp) return rcp; }
    char *pin = (char *)t->tie_pin;
    RL_HIP(hipMemcpyAsync(pin, c.st, sizeof(TreeState), hipMemcpyDeviceToHost, s));
    RL_HIP(hipMemcpyAsync(pin + sizeof(TreeState), c.nodes, (size_t)c.NC * sizeof(NodeRec), hipMemcpyDeviceToHost, s));
    RL_HIP(hipStreamSynchronize(s));
    TreeState st;
    memcpy(&st, pin, sizeof(st));
    if (!deferred && (st.stall_n <= 0 || st.stall_n > kSpec)) return fail(RL_ERR_STATE, "resolve_ties without a stalled tree (internal error)");
    nodes.resize((size_t)st.n_nodes);
    memcpy(nodes.data(), pin + sizeof(TreeState), nodes.size() * sizeof(NodeRec));
    todo.clear();
    if (deferred) { for (int x = 0; x < st.n_nodes; x++) if (nodes[x].left >= 0 && (nodes[x].tie & 0xc0) == 0x40) todo.push_back(x); }
    else for (int x = 0; x < st.stall_n; x++) todo.push_back(st.stall_node[x]);
    return RL_OK;
}

// ---- host planning: the derivation chains -------------------------------------------------------------------------------
struct TiePlan {
    int nx = 0, nA = 0, nv = 0, tiles = 0;           // nodes to resolve, chain nodes, nodes to verify; document tiles of the member compaction
    std::vector<TieNode> an; std::vector<TiePred> preds;      // chain nodes (directly accumulated), the split predicates of all paths
    std::vector<TieNode> vn; std::vector<int32_t> vx;         // nodes whose deferred cut is verified (k_tie_verify), and their index in the nodes to resolve
    std::vector<int32_t> xnode, xlen, xchain;        // [nx] node, [nx] chain length, [nx][chain_cap] chain nodes
    std::vector<long long> u0;                       // [nA] offset of a chain node's members in global member order
    size_t chain_cap = 1, list_total = 0, u_total = 0, fixed_bytes = 0;
    int maxcnt = 1;
    bool any_list = false;                           // a chain node other than the root: member lists are made
};

// the split predicates of node x's path from the root, appended bottom-up; returns how many
static int tie_push_path(const std::vector<NodeRec> &nodes, int x, std::vector<TiePred> &preds)
{
    int n = 0;
    for (int ch = x; nodes[ch].parent >= 0; ch = nodes[ch].parent, n++) {
        const NodeRec &P = nodes[nodes[ch].parent];
        preds.push_back(TiePred{P.best_f, P.best_t, P.pl == ch ? 1 : 0});
    }
    return n;
}

// no HIP call: only the sizes of c are read (N, F, TS)
static int tie_plan_chains(const Ctx &c, const std::vector<NodeRec> &nodes, const std::vector<int> &todo, bool deferred, TiePlan &pl)
{
    std::vector<TieNode> &an = pl.an; std::vector<TiePred> &preds = pl.preds;
    std::map<int, int> a_of;
    auto is_right = [&](int x) { return nodes[x].parent >= 0 && nodes[nodes[x].parent].pr == x; };
    auto direct = [&](int x) -> int {        // chain node of a directly accumulated node, with the split predicates of its path from the root
        auto it = a_of.find(x);
        if (it != a_of.end()) return it->second;
        TieNode A; A.node = x; A.pred0 = (int)preds.size(); A.is_root = (x == 0) ? 1 : 0; A.list0 = 0; A.count = nodes[x].gcount;
        A.gcount = nodes[x].gcount; A.pad = 0;             // count: this rank's members (the device sets it; == gcount on one GPU)
        A.npred = tie_push_path(nodes, x, preds);
        an.push_back(A);
        a_of[x] = (int)an.size() - 1;
        return (int)an.size() - 1;
    };
    const int nx = pl.nx = (int)todo.size();
    // deferred ties over several features: the node was cut by its first candidate; that every tied candidate cuts it the same way is verified
    // document by document (k_tie_verify) -- these are the nodes, with the split predicates of their paths
    if (deferred)
        for (int x = 0; x < nx; x++) {
            if ((nodes[todo[x]].tie & 3) != 2) continue;
            TieNode V; memset(&V, 0, sizeof(V));
            V.node = todo[x]; V.pred0 = (int)preds.size(); V.is_root = (todo[x] == 0) ? 1 : 0; V.gcount = nodes[todo[x]].gcount;
            V.npred = tie_push_path(nodes, todo[x], preds);
            pl.vn.push_back(V); pl.vx.push_back(x);
        }
    pl.nv = (int)pl.vn.size();
    std::vector<std::vector<int>> chains((size_t)nx);
    for (int x = 0; x < nx; x++) {
        // J(X): X itself when the Java accumulates it; else J(parent) - J(left sibling), the parent first (top-down)
        std::vector<int> subs;               // left siblings, bottom-up
        int cur = todo[x];
        while (is_right(cur)) { subs.push_back(nodes[nodes[cur].parent].pl); cur = nodes[cur].parent; }
        chains[x].push_back(direct(cur));
        for (auto it = subs.rbegin(); it != subs.rend(); ++it) chains[x].push_back(direct(*it));
        pl.chain_cap = std::max(pl.chain_cap, chains[x].size());
    }
    const int nA = pl.nA = (int)an.size();
    pl.u0.resize((size_t)nA);
    for (int i = 0; i < nA; i++) {
        TieNode &A = an[i];
        if (!A.is_root) { A.list0 = (int32_t)pl.list_total; pl.list_total += (size_t)std::min(A.gcount, c.N); pl.any_list = true; }
        pl.u0[i] = (long long)pl.u_total; pl.u_total += (size_t)A.gcount;
        pl.maxcnt = std::max(pl.maxcnt, std::min(A.gcount, c.N));
    }
    if (pl.list_total > ((size_t)1 << 31) - 1) return fail(RL_ERR_UNSUPPORTED, "tie-break: member lists beyond 2^31 entries");
    pl.xlen.resize((size_t)nx); pl.xchain.assign((size_t)nx * pl.chain_cap, 0); pl.xnode.resize((size_t)nx);
    for (int x = 0; x < nx; x++) {
        pl.xnode[x] = todo[x]; pl.xlen[x] = (int32_t)chains[x].size();
        for (size_t i = 0; i < chains[x].size(); i++) pl.xchain[(size_t)x * pl.chain_cap + i] = chains[x][i];
    }
    const int nv = pl.nv, tiles = pl.tiles = (c.N + kTieTile - 1) / kTieTile;
    // what tie_stage1 takes from the arena, array by array (rounded up: over-reservation is what keeps TieArena::used <= tie_cap true):
    //   tmask [nx][F][TS] bytes;  4-byte: need [nA][F], xf [nx][F], tile_cnt [nA][tiles], list [list_total + 1];  8-byte: jbin [nA][F][TS], jtot [nA];
    //   the blob: xchain, xnode + xlen, an, preds, u0 (+ the 256-byte alignment of every take);  nv > 0: vlist [nx][F][3], vcnt [nx + 1], the blob's vn + vx;
    //   fS [nx][F] + ft [nx][F]
    pl.fixed_bytes = (size_t)nx * c.F * c.TS + ((size_t)nA * c.F + (size_t)nx * c.F + (size_t)nA * tiles + pl.list_total + 64) * 4 + ((size_t)nA * c.F * c.TS + nA) * 8 +
                     (pl.xchain.size() + 2 * (size_t)nx + 16) * 4 + (size_t)nA * sizeof(TieNode) + (preds.size() + 1) * sizeof(TiePred) + (size_t)nA * 8 + 64 * 256 +
                     (nv > 0 ? (size_t)nx * c.F * 12 + (size_t)nx * 4 + (size_t)nv * (sizeof(TieNode) + 4) + 1024 : 0) + (size_t)nx * c.F * 12 + 1024;
    return RL_OK;
}

// ---- stage 1 on the device: fixed-size scratch, the tied candidates, the verification, the member lists ----------------
// Everything the later stages take from it.  tie_stage1 fills ALL of it from the arena as it stands when it runs, so running it again behind a
// move of the arena leaves no pointer into the old one anywhere.
struct TieStage1 {
    TieArgs a;                               // every kernel's view of the resolution
    TieArena ar;                             // the cursor behind stage 1's arrays: the evaluation takes its own from here on
    long long *d_u0 = nullptr;               // [nA] the plan's u0 (in the blob)
    int32_t *d_vflag = nullptr;              // nv > 0: a verified node is cut differently by one of its tied candidates (k_tie_verify)
    std::vector<int32_t> need, lcnt;         // [nA][F] feature f of chain node A is needed; [nA] this rank's members (zero when the walk was chosen up front)
};

static int tie_stage1(rl_trainer *t, const TiePlan &pl, bool walk_early, TieStage1 &s1)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const int nx = pl.nx, nA = pl.nA, nv = pl.nv, tiles = pl.tiles;
    // need[] and the chain nodes come back through the pinned buffer (the sharded gather's counts of all ranks later)
    { int rcp = tie_pin_reserve(t, (size_t)nA * c.F * sizeof(int32_t) + (size_t)nA * sizeof(TieNode) + (size_t)tie_ranks(t) * nA * sizeof(int32_t) + ((size_t)1 << 20)); if (rcp) return rcp; }
    s1 = TieStage1();
    s1.need.assign((size_t)nA * c.F, 0); s1.lcnt.assign((size_t)nA, 0);
    TieArena &ar = s1.ar; TieArgs &a = s1.a;
    ar.base = (char *)t->tie_buf; ar.cap = t->tie_cap;
    memset(&a, 0, sizeof(a));
    a.nx = nx; a.nA = nA; a.chain_cap = (int32_t)pl.chain_cap;
    TieBlob blob(t);
    const size_t o_xnode = blob.put(pl.xnode.data(), nx * sizeof(int32_t)), o_xlen = blob.put(pl.xlen.data(), nx * sizeof(int32_t)), o_xchain = blob.put(pl.xchain.data(), pl.xchain.size() * sizeof(int32_t));
    const size_t o_an = blob.put(pl.an.data(), nA * sizeof(TieNode)), o_preds = blob.put(pl.preds.data(), pl.preds.size() * sizeof(TiePred)), o_u0 = blob.put(pl.u0.data(), nA * sizeof(long long));
    const size_t o_vn = blob.put(pl.vn.data(), nv * sizeof(TieNode)), o_vx = blob.put(pl.vx.data(), nv * sizeof(int32_t));
    char *d_blob = nullptr;
    { int rcb = blob.upload(ar, s, &d_blob); if (rcb) return rcb; }
    a.an = (TieNode *)(d_blob + o_an);
    s1.d_u0 = (long long *)(d_blob + o_u0);
    a.tmask = ar.take<uint8_t>((size_t)nx * c.F * c.TS); a.need = ar.take<int32_t>((size_t)nA * c.F); a.xf = ar.take<int32_t>((size_t)nx * c.F);
    a.tile_cnt = ar.take<int32_t>((size_t)nA * tiles); a.list = ar.take<int32_t>(pl.list_total + 1);
    a.jbin = ar.take<double>((size_t)nA * c.F * c.TS); a.jtot = ar.take<double>(nA);
    a.fS = ar.take<double>((size_t)nx * c.F); a.ft = ar.take<int32_t>((size_t)nx * c.F);
    RL_HIP(hipMemsetAsync(a.need, 0, (size_t)nA * c.F * sizeof(int32_t), s));
    a.xnode = (int32_t *)(d_blob + o_xnode); a.xlen = (int32_t *)(d_blob + o_xlen); a.xchain = (int32_t *)(d_blob + o_xchain); a.preds = (TiePred *)(d_blob + o_preds);
    if (nv > 0) {
        a.vcnt = ar.take<int32_t>((size_t)nx + 1); a.vlist = ar.take<int32_t>((size_t)nx * c.F * 3);
        s1.d_vflag = a.vcnt + nx;
        RL_HIP(hipMemsetAsync(a.vcnt, 0, ((size_t)nx + 1) * sizeof(int32_t), s));
    }
    hipLaunchKernelGGL(k_tie_cand, dim3(c.F, nx), dim3(kFinThreads), 0, s, c, a);
    if (nv > 0) hipLaunchKernelGGL(k_tie_verify, dim3(tiles, nv), dim3(kThreads), 0, s, c, a, (const TieNode *)(d_blob + o_vn), (const int32_t *)(d_blob + o_vx), s1.d_vflag);
    if (pl.any_list) {
        hipLaunchKernelGGL(k_tie_count, dim3(tiles, nA), dim3(kThreads), 0, s, c, a, tiles);
        hipLaunchKernelGGL(k_tie_scan, dim3(nA), dim3(kThreads), 0, s, a, tiles);
        hipLaunchKernelGGL(k_tie_scatter, dim3(tiles, nA), dim3(kThreads), 0, s, c, a, tiles);
    }
    if (walk_early) return RL_OK;       // (need / lcnt stay zero: no pairs, the walk)
    char *pin = (char *)t->tie_pin;
    const size_t need_bytes = s1.need.size() * sizeof(int32_t);
    RL_HIP(hipMemcpyAsync(pin, a.need, need_bytes, hipMemcpyDeviceToHost, s));
    RL_HIP(hipMemcpyAsync(pin + need_bytes, a.an, (size_t)nA * sizeof(TieNode), hipMemcpyDeviceToHost, s));
    RL_HIP(hipStreamSynchronize(s));
    memcpy(s1.need.data(), pin, need_bytes);
    for (int i = 0; i < nA; i++) {      // this rank's member counts (k_tie_scan)
        TieNode A; memcpy(&A, pin + need_bytes + (size_t)i * sizeof(TieNode), sizeof(A));
        s1.lcnt[i] = pl.an[i].is_root ? c.N : (pl.any_list ? A.count : pl.an[i].gcount);
    }
    return RL_OK;
}

// ---- stage 2, host planning: the needed (chain node, feature) pairs, their bins' sizes, the chains and their segments ----
struct TieSpecPlan {
    std::vector<TiePair> pairs;
    std::vector<TieChain> chs; std::vector<int32_t> win_chain, chunk_chain;      // the contiguous chains; the chain of every window / chunk
    size_t v_total = 0, m_total = 0;         // values in vals[] (the chain nodes' members, then the pairs' sorted copies) / member bins in mb[]
    size_t l_u = 0, l_m = 0;                 // this rank's members of the chain nodes / of the pairs' chain nodes
    size_t spec_bytes = 0;
    int tiles_max = 1;

    void add_chain(long long off, int len, int out)
    {
        TieChain C; C.off = off; C.len = len; C.out = out; C.win0 = (int32_t)win_chain.size();
        C.win = std::min(16384, std::max(2048, ((len / 256 + 2047) / 2048) * 2048));
        const int nw = (len + C.win - 1) / C.win;
        for (int j = 0; j < nw; j++) win_chain.push_back((int32_t)chs.size());
        for (int j = 0; j <= nw; j++) chunk_chain.push_back((int32_t)chs.size());       // chunk ids: win0 + chain index + local chunk
        chs.push_back(C);
    }
};

// no HIP call
static void tie_plan_pairs(const Ctx &c, const TiePlan &pl, const std::vector<int32_t> &need, TieSpecPlan &sp)
{
    sp = TieSpecPlan();
    sp.v_total = pl.u_total;
    for (int i = 0; i < pl.nA; i++)
        for (int f = 0; f < c.F; f++)
            if (need[(size_t)i * c.F + f]) {
                TiePair P; P.a = i; P.f = f; P.tiles = (pl.an[i].gcount + kTsTile - 1) / kTsTile; P.pad = 0; P.v0 = (long long)sp.v_total; P.m0 = (long long)sp.m_total;
                sp.v_total += (size_t)pl.an[i].gcount; sp.m_total += (size_t)pl.an[i].gcount; sp.tiles_max = std::max(sp.tiles_max, P.tiles);
                sp.pairs.push_back(P);
            }
}

// cumulative bin counts of the pairs (exact): where every bin's run starts in the sorted values.  cnts [npairs][TS]; the tables' sizes once per trainer
static int tie_read_bin_counts(rl_trainer *t, const TiePlan &pl, const std::vector<TiePair> &pairs, std::vector<int32_t> &cnts)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const int npairs = (int)pairs.size();
    cnts.resize((size_t)npairs * c.TS);
    { int rcp = tie_pin_reserve(t, cnts.size() * sizeof(int32_t) + 4096); if (rcp) return rcp; }
    char *pin = (char *)t->tie_pin;
    for (int p = 0; p < npairs; p++)
        RL_HIP(hipMemcpyAsync(pin + (size_t)p * c.TS * sizeof(int32_t), c.cum_cnt + ((size_t)pl.an[pairs[p].a].node * c.F + pairs[p].f) * c.TS, (size_t)c.TS * sizeof(int32_t),
                              hipMemcpyDeviceToHost, s));
    RL_HIP(hipStreamSynchronize(s));
    memcpy(cnts.data(), pin, cnts.size() * sizeof(int32_t));
    if ((int)t->h_nthr.size() != c.F) { t->h_nthr.resize(c.F); RL_HIP(hipMemcpy(t->h_nthr.data(), c.nthr, c.F * sizeof(int32_t), hipMemcpyDeviceToHost)); }
    return RL_OK;
}

// no HIP call.  walk: no chains are laid out (cnts and nthr are not looked at); R > 1: sharded
static void tie_plan_spec(const Ctx &c, const TiePlan &pl, const std::vector<int32_t> &lcnt, const std::vector<int32_t> &cnts, const std::vector<int32_t> &nthr, bool walk, int R,
                          TieSpecPlan &sp)
{
    const int nA = pl.nA, npairs = (int)sp.pairs.size();
    const bool sharded = R > 1;
    if (!walk) {
        for (int i = 0; i < nA; i++) sp.add_chain(pl.u0[i], pl.an[i].gcount, -(i + 1));
        for (int p = 0; p < npairs; p++) {
            const TiePair &P = sp.pairs[p];
            const int32_t *cc = cnts.data() + (size_t)p * c.TS;
            for (int b = 0; b < nthr[P.f]; b++) {
                const int start = b > 0 ? cc[b - 1] : 0;
                sp.add_chain(P.v0 + start, cc[b] - start, (int)(((size_t)P.a * c.F + P.f) * c.TS + b));
            }
        }
    }
    const int nch = (int)sp.chs.size(), nwin = (int)sp.win_chain.size(), nchunks = (int)sp.chunk_chain.size(), tiles_max = sp.tiles_max;
    const size_t u_total = pl.u_total, v_total = sp.v_total, m_total = sp.m_total;
    size_t l_u = 0, l_m = 0;
    for (int i = 0; i < nA; i++) l_u += (size_t)lcnt[i];
    for (int p = 0; p < npairs; p++) l_m += (size_t)lcnt[sp.pairs[p].a];
    sp.l_u = l_u; sp.l_m = l_m;
    // what tie_eval_spec takes from the arena, array by array (rounded up, as fixed_bytes):
    //   mb [m_total + 64] 2-byte;  sharded (tie_gather_sharded): ul [l_u + 8] + urecv [u_total + 8] 8-byte, mbl [l_m + 8] + mbrecv [m_total + 8] 2-byte, lcnt [nA] + cntR [R][nA];
    //   lu0 [nA] + lm0 [npairs] (sharded) and the blob's m0 [npairs] 8-byte, pair_a [npairs];  vals [v_total + 1];  tbin [npairs][tiles_max][TS];
    //   per window: wsum + wpre (16 each), the blob's win_chain;  per chunk: cstart, cpre (16), centre (8), table [kSpW] (8 each), the blob's chunk_chain;
    //   per chain: cstate [4], ckey, cshift, the blob's TieChain;  the blob's pairs;  (+ the 256-byte alignment of every take)
    sp.spec_bytes = (m_total + 64) * 2 + (sharded ? (l_u + u_total + 64) * 8 + (l_m + m_total + 64) * 2 + (size_t)(R + 1) * nA * 4 : 0) + (size_t)(nA + 2 * npairs + 8) * 8 + v_total * 8 + (size_t)npairs * tiles_max * c.TS * 4 + (size_t)nwin * (16 + 16 + 4) + (size_t)nchunks * (4 + 16 + 8 + 8 * kSpW + 4) +
                    (size_t)nch * (16 + 8 + 8 + sizeof(TieChain)) + (size_t)npairs * sizeof(TiePair) + (size_t)(nwin + nchunks) * 4 + 64 * 256;
}

// ---- the memory decision --------------------------------------------------------------------------------------------------
// The contiguous chains need fixed_bytes + spec_bytes.  An arena that has to grow moves, so stage 1 runs again in the new one (and later
// resolutions ask for this much up front: tie_hint).  Out of memory: one GPU falls back to the literal walk (`walk` becomes true) in a minimal
// arena; a sharded run fails on every rank.
static int tie_reserve_spec(rl_trainer *t, const TiePlan &pl, const TieSpecPlan &sp, bool walk_early, bool &walk, TieStage1 &s1)
{
    hipStream_t s = t->stream;
    const size_t spec_need = pl.fixed_bytes + sp.spec_bytes + ((size_t)1 << 20);
    const bool grow = !walk && spec_need > t->tie_cap;
    int oom = 0;
    if (grow) {
        t->tie_hint = spec_need;
        if (tie_arena_reserve(t, t->tie_hint)) oom = 1;
    }
    if (tie_ranks(t) > 1) {
        // spec_bytes and the free memory differ from rank to rank, the exchange of the gather does not: the out-of-memory decision is taken by ALL
        // ranks (a rank that fell back to the walk on its own would leave the others waiting in the all-to-all -- and the walk sums its own
        // documents only).  One 4-byte all-reduce per resolution of a sharded run.
        if (!t->d_tie_flag) RL_HIP(t->pool.alloc(&t->d_tie_flag, (size_t)4));
        int32_t *d_oom = t->d_tie_flag;
        RL_HIP(hipMemcpyAsync(d_oom, &oom, sizeof(oom), hipMemcpyHostToDevice, s));
        int rcd = t->dist->allreduce(d_oom, 1, DT_I32, OP_MAX, s);
        if (rcd) return rcd;
        int32_t any = 0;
        RL_HIP(hipMemcpyAsync(&any, d_oom, sizeof(any), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        if (any) return fail(RL_ERR_HIP, "tie-break: out of device memory on a rank of the job (the sharded tie-break needs the gathered chains on every rank)");
    } else if (grow && oom) {      // no room for the contiguous chains: the literal walk in a minimal arena
        walk = true;
        if (tie_arena_reserve(t, pl.fixed_bytes + ((size_t)1 << 20))) return fail(RL_ERR_HIP, "tie-break: out of device memory");
    }
    return grow ? tie_stage1(t, pl, walk_early, s1) : RL_OK;
}

// ---- the evaluation: sequential per-bin sums of the needed (chain node, feature) rows, in the Java's order --------------
// the literal walk: one kernel, this rank's documents in ascending order
static int tie_eval_walk(rl_trainer *t, const TiePlan &pl, const TieStage1 &s1)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const int nbg = (c.TS + 63) / 64;
    RL_HIP(hipMemsetAsync(s1.a.jbin, 0, (size_t)pl.nA * c.F * c.TS * sizeof(double), s));
    hipLaunchKernelGGL(k_tie_jsum, dim3(c.F, nbg + 1, pl.nA), dim3(64), 0, s, c, s1.a, nbg);
    return RL_OK;
}

// one GPU: this rank's members ARE the members -- lambda and bins go straight to their global places
static void tie_gather_local(rl_trainer *t, const TiePlan &pl, const TieStage1 &s1, const SpArgs &sp, const long long *d_m0)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const int gx = std::min(4096, (pl.maxcnt + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_tie_gather, dim3(gx, pl.nA), dim3(kThreads), 0, s, c, s1.a, sp.vals, (const long long *)s1.d_u0);
    if (sp.npairs > 0) hipLaunchKernelGGL(k_tie_gather_bins, dim3(gx, sp.npairs), dim3(kThreads), 0, s, c, s1.a, sp.pairs, sp.mb, d_m0);
}

// sharded: rank order is global document order, so the global arrays are the ranks' pieces behind each other.  Every rank gathers its own
// pieces, all ranks exchange them (an all-gather of variable pieces through the all-to-all primitive), and every rank then runs the SAME
// evaluation on the same global arrays -- the decision is rank-invariant by construction.
static int tie_gather_sharded(rl_trainer *t, const TiePlan &pl, const TieSpecPlan &spl, TieStage1 &s1, const SpArgs &sp, const long long *d_m0, const int32_t *d_paira)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    TieArena &ar = s1.ar;
    const int nA = pl.nA, npairs = sp.npairs, R = tie_ranks(t);
    const size_t l_u = spl.l_u, l_m = spl.l_m, u_total = pl.u_total, m_total = spl.m_total;
    const std::vector<TiePair> &pairs = spl.pairs; const std::vector<int32_t> &lcnt = s1.lcnt;
    std::vector<long long> lu0((size_t)nA), lm0((size_t)std::max(npairs, 1));
    { long long o = 0; for (int i = 0; i < nA; i++) { lu0[i] = o; o += lcnt[i]; } }
    { long long o = 0; for (int p2 = 0; p2 < npairs; p2++) { lm0[p2] = o; o += lcnt[pairs[p2].a]; } }
    long long *d_lu0 = ar.take<long long>(nA), *d_lm0 = ar.take<long long>(std::max(npairs, 1));
    int32_t *d_lcnt = ar.take<int32_t>(nA), *d_cntR = ar.take<int32_t>((size_t)R * nA);
    double *d_ul = ar.take<double>(l_u + 8), *d_urecv = ar.take<double>(u_total + 8);
    uint16_t *d_mbl = ar.take<uint16_t>(l_m + 8), *d_mbrecv = ar.take<uint16_t>(m_total + 8);
    if (ar.used > t->tie_cap) return fail(RL_ERR_HIP, "tie-break: scratch arena too small (internal error)");
    RL_HIP(hipMemcpyAsync(d_lu0, lu0.data(), nA * sizeof(long long), hipMemcpyHostToDevice, s));
    if (npairs > 0) RL_HIP(hipMemcpyAsync(d_lm0, lm0.data(), npairs * sizeof(long long), hipMemcpyHostToDevice, s));
    RL_HIP(hipMemcpyAsync(d_lcnt, lcnt.data(), nA * sizeof(int32_t), hipMemcpyHostToDevice, s));
    const int gx = std::min(4096, (pl.maxcnt + kThreads - 1) / kThreads);
    hipLaunchKernelGGL(k_tie_gather, dim3(gx, nA), dim3(kThreads), 0, s, c, s1.a, d_ul, (const long long *)d_lu0);
    if (npairs > 0) hipLaunchKernelGGL(k_tie_gather_bins, dim3(gx, npairs), dim3(kThreads), 0, s, c, s1.a, sp.pairs, d_mbl, (const long long *)d_lm0);
    int rcd = t->dist->allgather(d_lcnt, d_cntR, (size_t)nA * sizeof(int32_t), s);
    if (rcd) return rcd;
    std::vector<int32_t> cntR((size_t)R * nA);
    { int rcp = tie_pin_reserve(t, cntR.size() * sizeof(int32_t)); if (rcp) return rcp; }
    char *pin = (char *)t->tie_pin;
    RL_HIP(hipMemcpyAsync(pin, d_cntR, cntR.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RL_HIP(hipStreamSynchronize(s));
    memcpy(cntR.data(), pin, cntR.size() * sizeof(int32_t));
    std::vector<int64_t> scount(R), sdispl(R, 0), rcount(R), rdispl(R);
    {   // lambda pieces
        int64_t o = 0;
        for (int r = 0; r < R; r++) { int64_t n = 0; for (int i = 0; i < nA; i++) n += cntR[(size_t)r * nA + i]; rcount[r] = n * 8; rdispl[r] = o; o += n * 8; scount[r] = (int64_t)l_u * 8; }
        if ((size_t)o != u_total * 8) return fail(RL_ERR_COMM, "tie-break: the ranks' member counts do not add up to the nodes' document counts");
        rcd = t->dist->alltoallv(d_ul, scount.data(), sdispl.data(), d_urecv, rcount.data(), rdispl.data(), s);
        if (rcd) return rcd;
        hipLaunchKernelGGL(k_tie_place<double>, dim3(nA, R), dim3(kThreads), 0, s, (const double *)d_urecv, sp.vals, (const int32_t *)d_cntR, (const int32_t *)nullptr,
                           (const long long *)s1.d_u0, nA, nA, R);
    }
    if (npairs > 0) {   // bins of the pairs
        int64_t o = 0;
        for (int r = 0; r < R; r++) { int64_t n = 0; for (int p2 = 0; p2 < npairs; p2++) n += cntR[(size_t)r * nA + pairs[p2].a]; rcount[r] = n * 2; rdispl[r] = o; o += n * 2; scount[r] = (int64_t)l_m * 2; }
        rcd = t->dist->alltoallv(d_mbl, scount.data(), sdispl.data(), d_mbrecv, rcount.data(), rdispl.data(), s);
        if (rcd) return rcd;
        hipLaunchKernelGGL(k_tie_place<uint16_t>, dim3(npairs, R), dim3(kThreads), 0, s, (const uint16_t *)d_mbrecv, sp.mb, (const int32_t *)d_cntR, d_paira, d_m0, npairs, nA, R);
    }
    return RL_OK;
}

// the contiguous speculative chains: every chain node's values in global member order, every pair's sorted by bin (k_ts_*: a stable sort, so
// every bin's run keeps the members' order), then all chains at once (k_sp_*, rl_tie.inc)
static int tie_eval_spec(rl_trainer *t, const TiePlan &pl, const TieSpecPlan &spl, TieStage1 &s1)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    TieArena &ar = s1.ar; const TieArgs &a = s1.a;
    const int nch = (int)spl.chs.size(), nwin = (int)spl.win_chain.size(), nchunks = (int)spl.chunk_chain.size(), npairs = (int)spl.pairs.size();
    const int tiles_max = spl.tiles_max, nbg = (c.TS + 63) / 64;
    SpArgs sp; memset(&sp, 0, sizeof(sp));
    sp.nchains = nch; sp.nwin = nwin; sp.nchunks = nchunks; sp.npairs = npairs; sp.tiles_max = tiles_max;
    TieBlob blob(t);
    const size_t o_pairs = blob.put(spl.pairs.data(), npairs * sizeof(TiePair)), o_chs = blob.put(spl.chs.data(), nch * sizeof(TieChain));
    const size_t o_winc = blob.put(spl.win_chain.data(), nwin * sizeof(int32_t)), o_chunkc = blob.put(spl.chunk_chain.data(), nchunks * sizeof(int32_t));
    std::vector<long long> m0s((size_t)npairs); std::vector<int32_t> pair_a((size_t)npairs);
    for (int p2 = 0; p2 < npairs; p2++) { m0s[p2] = spl.pairs[p2].m0; pair_a[p2] = spl.pairs[p2].a; }
    const size_t o_m0 = blob.put(m0s.data(), npairs * sizeof(long long)), o_paira = blob.put(pair_a.data(), npairs * sizeof(int32_t));
    char *d_blob = nullptr;
    { int rcb = blob.upload(ar, s, &d_blob); if (rcb) return rcb; }
    sp.vals = ar.take<double>(spl.v_total + 1); sp.tbin = ar.take<int32_t>((size_t)npairs * tiles_max * c.TS);
    sp.wsum = ar.take<double2>(nwin + 1); sp.wpre = ar.take<double2>(nwin + 1);
    sp.cstart = ar.take<int32_t>(nchunks + 1); sp.cpre = ar.take<double2>(nchunks + 1);
    sp.centre = ar.take<unsigned long long>(nchunks + 1); sp.table = ar.take<unsigned long long>((size_t)nchunks * kSpW + 1);
    sp.cstate = ar.take<int32_t>((size_t)nch * 4); sp.ckey = ar.take<unsigned long long>(nch); sp.cshift = ar.take<double>(nch);
    sp.open = ar.take<int32_t>(4);
    sp.pairs = (TiePair *)(d_blob + o_pairs); sp.chains = (TieChain *)(d_blob + o_chs); sp.win_chain = (int32_t *)(d_blob + o_winc); sp.chunk_chain = (int32_t *)(d_blob + o_chunkc);
    sp.u0 = s1.d_u0;
    sp.mb = ar.take<uint16_t>(spl.m_total + 64);
    if (ar.used > t->tie_cap) return fail(RL_ERR_HIP, "tie-break: scratch arena too small (internal error)");
    const long long *d_m0 = (const long long *)(d_blob + o_m0);
    if (tie_ranks(t) == 1) tie_gather_local(t, pl, s1, sp, d_m0);
    else { int rcg = tie_gather_sharded(t, pl, spl, s1, sp, d_m0, (const int32_t *)(d_blob + o_paira)); if (rcg) return rcg; }
    hipLaunchKernelGGL(k_ts_count, dim3(tiles_max, npairs), dim3(kThreads), (size_t)c.TS * 4, s, c, a, sp);
    hipLaunchKernelGGL(k_ts_scan, dim3(npairs, nbg), dim3(64), 0, s, c, a, sp);
    hipLaunchKernelGGL(k_ts_scatter, dim3(tiles_max, npairs), dim3(kTsWaves * 64), (size_t)kTsWaves * c.TS * 4, s, c, a, sp);
    const int cb = (nch + kThreads - 1) / kThreads;
    if (nwin > 0) hipLaunchKernelGGL(k_sp_sum, dim3(nwin), dim3(64), 0, s, sp);
    hipLaunchKernelGGL(k_sp_scan, dim3(cb), dim3(kThreads), 0, s, sp);
    if (nwin > 0) hipLaunchKernelGGL(k_sp_bounds, dim3(nwin), dim3(64), 0, s, sp);
    hipLaunchKernelGGL(k_sp_run<false>, dim3(nchunks), dim3(kSpW), 0, s, sp);
    hipLaunchKernelGGL(k_sp_drift, dim3(cb), dim3(kThreads), 0, s, sp);
    hipLaunchKernelGGL(k_sp_run<false>, dim3(nchunks), dim3(kSpW), 0, s, sp);
    { int rcp = tie_pin_reserve(t, sizeof(int32_t)); if (rcp) return rcp; }
    char *pin = (char *)t->tie_pin;
    int32_t open = 0;
    for (int rep = 0; rep <= kSpRepairs; rep++) {
        RL_HIP(hipMemsetAsync(sp.open, 0, sizeof(int32_t), s));
        hipLaunchKernelGGL(k_sp_stitch, dim3(cb), dim3(kThreads), 0, s, sp, a, rep == kSpRepairs ? 1 : 0);
        RL_HIP(hipMemcpyAsync(pin, sp.open, sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        memcpy(&open, pin, sizeof(open));
        if (open == 0) break;
        t->tie_spec_repairs++;
        hipLaunchKernelGGL(k_sp_run<true>, dim3(nchunks), dim3(kSpW), 0, s, sp);
    }
    if (c.steplog) {       // debug statistics (RLHIP_STEPLOG): window misses / serial chunks of this resolution
        std::vector<int32_t> cst((size_t)nch * 4);
        RL_HIP(hipMemcpyAsync(cst.data(), sp.cstate, cst.size() * sizeof(int32_t), hipMemcpyDeviceToHost, s));
        RL_HIP(hipStreamSynchronize(s));
        for (int i = 0; i < nch; i++) { t->tie_spec_miss += cst[4 * (size_t)i + 1]; t->tie_spec_serial += cst[4 * (size_t)i + 2]; }
    }
    t->tie_spec_segs += nchunks;
    return RL_OK;
}

// ---- the commit -------------------------------------------------------------------------------------------------------------
// prefixes of all needed rows at once, the tied candidates of all (feature, node) pairs at once, then one block: arg-max, node records, select_step
static int tie_commit(rl_trainer *t, const TiePlan &pl, const TieStage1 &s1, size_t fin_lds, int nodes_in_lds, bool deferred, bool *other_cut)
{
    const Ctx &c = t->ctx;
    hipStream_t s = t->stream;
    const int nx = pl.nx, nA = pl.nA, nv = pl.nv;
    hipLaunchKernelGGL(k_tie_prefix, dim3(c.F, nA), dim3(64), (size_t)c.TS * 8, s, c, s1.a);
    hipLaunchKernelGGL(k_tie_eval, dim3(c.F, nx), dim3(kFinThreads), 0, s, c, s1.a);
    hipLaunchKernelGGL(k_tie_finish, dim3(1), dim3(kFinThreads), fin_lds, s, c, s1.a, nodes_in_lds, deferred ? 1 : 0);
    RL_HIP(hipGetLastError());
    if (nv > 0 && tie_ranks(t) > 1) {      // every rank checked its own documents: a cut that differs anywhere makes every rank grow the tree again
        int rcd = t->dist->allreduce(s1.d_vflag, 1, DT_I32, OP_MAX, s);
        if (rcd) return rcd;
    }
    { int rcp = tie_pin_reserve(t, sizeof(int32_t)); if (rcp) return rcp; }
    char *pin = (char *)t->tie_pin;
    if (nv > 0) RL_HIP(hipMemcpyAsync(pin, s1.d_vflag, sizeof(int32_t), hipMemcpyDeviceToHost, s));
    RL_HIP(hipStreamSynchronize(s));
    if (nv > 0 && other_cut) { int32_t fl = 0; memcpy(&fl, pin, sizeof(fl)); *other_cut = (fl != 0) || t->knobs.tie_force_regrow; }
    t->tie_stalls++; t->tie_nodes += nx; t->tie_chain_nodes += nA; if (deferred) t->tie_batches++;
    for (auto &A : pl.an) t->tie_chain_docs += A.count;
    return RL_OK;
}

// deferred = false: the tree is stalled on TreeState::stall_node (ties whose candidates may cut the node differently); afterwards the growth resumes.
// deferred = true: the tree is grown; the committed nodes flagged 0x40 (plateau ties of right children: the partition was known, the stored
// threshold was not) get the Java's threshold, all of them in one batch, before the tree is exported.
static int resolve_ties(rl_trainer *t, size_t fin_lds, int nodes_in_lds, bool deferred = false, bool *other_cut = nullptr)
{
    const Ctx &c = t->ctx;
    const auto t_begin = std::chrono::steady_clock::now();
    struct TieScope { DistBackend *d; TieScope(DistBackend *d_) : d(d_) { if (d) d->tie_scope = true; } ~TieScope() { if (d) d->tie_scope = false; } } tie_scope(t->dist.get());
    auto t_last = t_begin;       // knobs.tie_prof: host microseconds per phase
    auto mark = [&](int ph) { if (!t->knobs.tie_prof) return; const auto now = std::chrono::steady_clock::now(); t->tie_phase_us[ph] += (long long)std::chrono::duration_cast<std::chrono::microseconds>(now - t_last).count(); t_last = now; };
    int rc;
    std::vector<NodeRec> nodes; std::vector<int> todo;
    if ((rc = tie_read_tree(t, deferred, nodes, todo))) return rc;
    mark(0);
    if (todo.empty()) return RL_OK;
    TiePlan pl;
    if ((rc = tie_plan_chains(c, nodes, todo, deferred, pl))) return rc;
    const int R = tie_ranks(t);
    const bool huge_tables = (size_t)kTsWaves * c.TS * 4 > (size_t)60 * 1024;      // the sort's cursors would not fit the LDS
    // short chains: the literal walk (one kernel, ~6 ns a document) beats the dozen launches and two more host round trips of the contiguous-chain path;
    // known before anything ran on the device, so stage 1 does not have to report back either
    const bool walk_early = R == 1 && (t->knobs.tie_walk || pl.u_total <= t->knobs.tie_walk_max || huge_tables);
    if (tie_arena_reserve(t, std::max(pl.fixed_bytes + t->knobs.tie_slack, t->tie_hint))) return fail(RL_ERR_HIP, "tie-break: out of device memory");
    mark(1);
    TieStage1 s1;
    if ((rc = tie_stage1(t, pl, walk_early, s1))) return rc;
    mark(2);
    TieSpecPlan spl;
    tie_plan_pairs(c, pl, s1.need, spl);
    // the walk reads this rank's documents only: never on a sharded run (rl_init keeps the tie-break off for sharded runs with huge tables)
    bool walk = R == 1 && (walk_early || spl.pairs.empty() || huge_tables);
    std::vector<int32_t> cnts;
    if (!walk && (rc = tie_read_bin_counts(t, pl, spl.pairs, cnts))) return rc;
    tie_plan_spec(c, pl, s1.lcnt, cnts, t->h_nthr, walk, R, spl);
    if ((rc = tie_reserve_spec(t, pl, spl, walk_early, walk, s1))) return rc;
    if ((rc = walk ? tie_eval_walk(t, pl, s1) : tie_eval_spec(t, pl, spl, s1))) return rc;
    mark(3);
    if ((rc = tie_commit(t, pl, s1, fin_lds, nodes_in_lds, deferred, other_cut))) return rc;
    mark(4);
    t->tie_us += (long long)std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now() - t_begin).count();
    return RL_OK;
}

}  // namespace rl
