// dist.cpp — multi-GPU allreduce: one process per GPU, RCCL point-to-point.
//
// The per-rank step program is the reference's per-core dataflow program
// (allred_BO_2D/kernels/dataflow_kernel.cpp) with the NoC replaced by xGMI:
//   reduce-scatter step k (:152-213): send the blocks of send_mask_k to the
//     partner, receive recv_mask_k's blocks into a staging buffer, add them
//     into the local bucket (compute_kernel.cpp:35-67);
//   all-gather step k, reverse order (:219-267): send the blocks of
//     recv_mask_k, receive the partner's owned blocks straight into the bucket;
//   LO (shouldSendBlock with bandwidth_optimal = 0, :19-29): full-vector
//     exchange + add every step.
// A step's blocks go out as one ncclSend/ncclRecv per contiguous run of set
// bits, inside one ncclGroupStart/End, on the caller's stream; the add of every
// received run of every channel is ONE HIP kernel launch (k_add_segs) on the
// same stream.  A rank's program is built once per (desc, rank) and cached
// (the 2-128 kB latency regime of BASELINE config 5 pays no host rebuild per
// call).  The identical program also
// runs on host memory with a caller-supplied exchange (allred_dist_allreduce_host)
// so CPU tests (gloo) cover every step of it.
#include <hip/hip_runtime.h>
#include <rccl/rccl.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <condition_variable>
#include <map>
#include <memory>
#include <mutex>
#include <thread>
#include <tuple>
#include <vector>

#include "internal.hpp"

using namespace tsa;

struct allred_comm {
    ncclComm_t comm = nullptr;
    int nranks = 0, rank = 0, device = 0;
    // bounded RCCL: non-blocking communicator, polled against a deadline; aborted
    // past it (every later call then returns ALLRED_ERR_TRANSPORT)
    int timeout_ms = 0;             // 0 = default_timeout_ms()
    bool aborted = false;
    uint64_t connected = 0;         // peers this communicator has exchanged with (RCCL set their connections up)
    const std::atomic<int>* cancel = nullptr;   // run_multi_gpu: another GPU's thread failed
    // allred_dist_allreduce_pipelined: the bucket started by the last call (its rows are
    // written by the next call or the flush) and its allreduced partial in the workspace
    uint64_t calls = 0;             // allred_dist_allreduce calls (the hierarchical partial alternates halves)
    uint16_t* pend = nullptr;
    uint16_t* pend_partial = nullptr;
    int pend_parity = 0, pend_local = 0;
    size_t pend_elems = 0;
};

namespace {

struct Seg {
    size_t off, len;  // elements
};

// One exchange with one peer inside a step.
struct Exch {
    int peer = -1;
    std::vector<Seg> send;          // from the bucket
    std::vector<Seg> recv;          // into staging (add) or into the bucket (AG)
    bool recv_to_bucket = false;
    bool add = false;               // bucket[recv segs] += staging[recv segs]
    size_t blk = 0;                 // block size of this exchange's channel (elements)
    size_t base = 0;                // channel slice start (elements)
};

// A step = the exchanges of every channel, issued as one RCCL group, then one
// add launch over every received segment (elements) of every channel.
struct Step {
    std::vector<Exch> ex;
    std::vector<uint64_t> add_off, add_len;
};

void runs(uint64_t mask, int total, size_t blk, size_t base, std::vector<Seg>* out) {
    int b = 0;
    while (b < total) {
        if (!((mask >> b) & 1ull)) { ++b; continue; }
        int e = b;
        while (e < total && ((mask >> e) & 1ull)) ++e;
        out->push_back(Seg{base + (size_t)b * blk, (size_t)(e - b) * blk});
        b = e;
    }
}

// ---- link-spreading channels ---------------------------------------------
// On the GPU grids (2,2), (2,4), (4,8) both schedules are XOR schedules:
// partner_k(x) = x ^ m_k with (m_0 .. m_{S-1}) a basis of GF(2)^S (Swing 4x2:
// 1, 4, 3; RecDub 4x2: 1, 4, 2).  Channel c relabels rank r as x = a^c * r in
// GF(2^S) (a = the primitive element), so its step-k partner is
// r ^ a^-c * m_k: at every step the 2^S - 1 channels use 2^S - 1 distinct
// masks = every peer of the full xGMI mesh at once.  Each channel
// allreduces its own slice of the bucket with the unmodified schedule in the
// relabeled ids, so every slice is an exact BO (or LO) allreduce.
int gf_mul(int a, int b, int S) {
    static const int poly[4] = {0, 0x3, 0x7, 0xb};  // x+1 (trivial), x^2+x+1, x^3+x+1
    int r = 0;
    for (int i = 0; i < S; ++i)
        if ((b >> i) & 1) r ^= a << i;
    for (int i = 2 * S - 2; i >= S; --i)
        if ((r >> i) & 1) r ^= poly[S] << (i - S);
    return r;
}

int gf_pow_alpha(int c, int S) {  // a^c, a = x (= 2) for S >= 2; a = 1 for S = 1
    int v = 1;
    for (int i = 0; i < c; ++i) v = S >= 2 ? gf_mul(v, 2, S) : 1;
    return v;
}

// channels usable on this schedule: 2^S - 1 for an XOR schedule with S <= 3, else 1
int max_channels(const allred_schedule& s) {
    if (s.steps < 1 || s.steps > 3) return 1;
    for (int k = 0; k < s.steps; ++k) {
        const int m = s.partner[0][k];
        for (int x = 0; x < s.total; ++x)
            if (s.partner[x][k] != (x ^ m)) return 1;
    }
    return (1 << s.steps) - 1;
}

int channels_for(const allred_schedule& s, int requested, size_t n) {
    const int cmax = max_channels(s);
    if (requested > 0) return requested < cmax ? requested : cmax;
    // auto: spread buckets of >= 1 MiB over every link; small ones stay latency-optimal
    return n * 2 >= (1u << 20) ? cmax : 1;
}

// slice of channel c: whole units of 8*N elements (keeps blocks 16-byte aligned)
void slice_of(size_t n, int N, int C, int c, size_t* base, size_t* len) {
    const size_t unit = 8 * (size_t)N, units = n / unit;
    const size_t q = units / C, r = units % C;
    const size_t before = q * c + (c < (int)r ? c : r);
    *base = before * unit;
    *len = (q + (c < (int)r ? 1 : 0)) * unit;
}

// the rank's program (LO: n need only be a multiple of 8; one channel)
std::vector<Step> program(const allred_schedule& s, int rank, int variant, size_t n, int C) {
    const int N = s.total, S = s.steps;
    if (variant == ALLRED_LO && n % (8 * (size_t)N)) C = 1;
    std::vector<Step> prog;
    auto chan = [&](int c, size_t* base, size_t* len) {
        if (C == 1) { *base = 0; *len = n; return; }
        slice_of(n, N, C, c, base, len);
    };
    auto id_of = [&](int c, int r) { return C == 1 ? r : gf_mul(gf_pow_alpha(c, S), r, S); };
    // peer of real rank r on channel c at step k: the real rank whose relabel is partner(x, k)
    auto peer_of = [&](int c, int r, int k) {
        const int x = id_of(c, r);
        const int px = s.partner[x][k];
        if (C == 1) return px;
        for (int q = 0; q < N; ++q)
            if (id_of(c, q) == px) return q;
        return -1;
    };
    if (variant == ALLRED_LO) {
        for (int k = 0; k < S; ++k) {
            Step st;
            for (int c = 0; c < C; ++c) {
                size_t base, len;
                chan(c, &base, &len);
                if (!len) continue;
                Exch e;
                e.peer = peer_of(c, rank, k);
                e.send.push_back(Seg{base, len});
                e.recv.push_back(Seg{base, len});
                e.add = true;
                e.base = base;
                e.blk = len;
                st.add_off.push_back(base);
                st.add_len.push_back(len);
                st.ex.push_back(e);
            }
            prog.push_back(st);
        }
        return prog;
    }
    for (int k = 0; k < S; ++k) {  // reduce-scatter
        Step st;
        for (int c = 0; c < C; ++c) {
            size_t base, len;
            chan(c, &base, &len);
            if (!len) continue;
            const int x = id_of(c, rank);
            Exch e;
            e.peer = peer_of(c, rank, k);
            e.blk = len / (size_t)N;
            e.base = base;
            runs(s.send[x][k], N, e.blk, base, &e.send);
            runs(s.recv[x][k], N, e.blk, base, &e.recv);
            e.add = true;
            for (const Seg& g : e.recv) {
                st.add_off.push_back(g.off);
                st.add_len.push_back(g.len);
            }
            st.ex.push_back(e);
        }
        prog.push_back(st);
    }
    for (int k = S - 1; k >= 0; --k) {  // all-gather
        Step st;
        for (int c = 0; c < C; ++c) {
            size_t base, len;
            chan(c, &base, &len);
            if (!len) continue;
            const int x = id_of(c, rank);
            Exch e;
            e.peer = peer_of(c, rank, k);
            e.blk = len / (size_t)N;
            e.base = base;
            runs(s.recv[x][k], N, e.blk, base, &e.send);
            runs(s.send[x][k], N, e.blk, base, &e.recv);
            e.recv_to_bucket = true;
            st.ex.push_back(e);
        }
        prog.push_back(st);
    }
    return prog;
}

// the rank's program for desc, built once and cached (key: every desc field that
// shapes it, the channel count actually used, the rank)
using ProgKey = std::tuple<int, int, int, int, uint64_t, int, int>;
constexpr size_t kMaxCachedPrograms = 1024;   // per-(desc, rank) programs / verdicts kept
std::mutex g_prog_mu;
std::map<ProgKey, std::shared_ptr<const std::vector<Step>>> g_progs;

std::shared_ptr<const std::vector<Step>> cached_program(const allred_dist_desc* d, const allred_schedule& s, int rank,
                                                        int C) {
    const ProgKey key{d->algo, d->variant, d->side_length, d->total_nodes, d->elems, C, rank};
    std::lock_guard<std::mutex> g(g_prog_mu);
    auto it = g_progs.find(key);
    // bounded: a job cycling through many bucket sizes starts the cache afresh
    // (programs in use stay alive through their shared_ptr)
    if (it == g_progs.end() && g_progs.size() >= kMaxCachedPrograms) g_progs.clear();
    if (it == g_progs.end())
        it = g_progs.emplace(key, std::make_shared<const std::vector<Step>>(
                                      program(s, rank, d->variant, (size_t)d->elems, C))).first;
    return it->second;
}

int add_launches(const Step& st) { return ((int)st.add_off.size() + kMaxAddSegs - 1) / kMaxAddSegs; }

// ---- check mode (tune "check" = 1; SURVEY §5: the reference has no race or
// invariant checking, its semaphore protocol hangs on a wrong config) --------
// verify_program: rank's program against every partner's, step by step —
// what a partner sends at step k is exactly what this rank receives from it
// at step k (same offsets and lengths, channel by channel), the received runs
// of a step are disjoint and inside the bucket, and only reduce-scatter / LO
// receives are added.  Verified once per (desc, rank) and remembered.
// Poisoning (in both executors): every receive region is filled with 0xFFFF (a
// bf16 quiet NaN) before its step, so an element the transport never delivered
// cannot pass as data — it turns the result into NaN instead of stale bytes.
constexpr uint16_t kPoison = 0xFFFF;

// The part of a rank's cached program a call runs: all of it (the allreduce), or one half of
// the BO program — its first S steps are the reduce-scatter, its last S the all-gather
// (allred_dist_reduce_scatter / allred_dist_all_gather run a slice of the same vector).
enum Part { kWhole = 0, kReduceScatter = 1, kAllGather = 2 };
void part_range(Part part, size_t steps, size_t* first, size_t* last) {
    *first = part == kAllGather ? steps / 2 : 0;
    *last = part == kReduceScatter ? steps / 2 : steps;
}

// the verdicts of a (desc, rank), one per part (0: not verified yet, else status + 1)
struct Verdicts {
    int st1[3] = {0, 0, 0};
};
std::mutex g_verified_mu;
std::map<ProgKey, Verdicts> g_verified;

int verify_program(const allred_dist_desc* d, const allred_schedule& s, int rank, int C, Part part = kWhole) {
    const ProgKey key{d->algo, d->variant, d->side_length, d->total_nodes, d->elems, C, rank};
    {
        std::lock_guard<std::mutex> g(g_verified_mu);
        const auto it = g_verified.find(key);
        if (it != g_verified.end() && it->second.st1[part]) return it->second.st1[part] - 1;
    }
    const size_t n = (size_t)d->elems;
    const auto mine = cached_program(d, s, rank, C);
    int st = ALLRED_OK;
    size_t first, last;
    part_range(part, mine->size(), &first, &last);
    for (size_t k = first; k < last && st == ALLRED_OK; ++k) {   // only the steps that run
        const Step& step = (*mine)[k];
        std::vector<Seg> all;
        for (size_t x = 0; x < step.ex.size() && st == ALLRED_OK; ++x) {
            const Exch& e = step.ex[x];
            if (e.peer < 0 || e.peer >= d->total_nodes || e.peer == rank) { st = ALLRED_ERR_SCHEDULE; break; }
            if (e.add == e.recv_to_bucket) { st = ALLRED_ERR_SCHEDULE; break; }
            const auto theirs = cached_program(d, s, e.peer, C);
            if (theirs->size() != mine->size() || (*theirs)[k].ex.size() != step.ex.size()) { st = ALLRED_ERR_SCHEDULE; break; }
            const Exch& f = (*theirs)[k].ex[x];   // the same channel's exchange at the partner
            if (f.peer != rank || f.send.size() != e.recv.size() || e.send.size() != f.recv.size()) {
                st = ALLRED_ERR_SCHEDULE;
                break;
            }
            for (size_t i = 0; i < e.recv.size(); ++i)
                if (f.send[i].off != e.recv[i].off || f.send[i].len != e.recv[i].len) st = ALLRED_ERR_SCHEDULE;
            for (const Seg& g : e.recv) {
                if (g.off + g.len > n) st = ALLRED_ERR_SCHEDULE;
                all.push_back(g);
            }
        }
        std::sort(all.begin(), all.end(), [](const Seg& a, const Seg& b) { return a.off < b.off; });
        for (size_t i = 1; i < all.size(); ++i)
            if (all[i - 1].off + all[i - 1].len > all[i].off) st = ALLRED_ERR_SCHEDULE;
    }
    std::lock_guard<std::mutex> g(g_verified_mu);
    if (g_verified.size() >= kMaxCachedPrograms) g_verified.clear();
    g_verified[key].st1[part] = st + 1;
    return st;
}

int check_desc(const allred_dist_desc* d, allred_schedule* s) {
    if (!d) return ALLRED_ERR_ARG;
    if (d->variant != ALLRED_BO && d->variant != ALLRED_LO && d->variant != ALLRED_MEM) return ALLRED_ERR_UNSUPPORTED;
    // mem_2D over RCCL: one rank per GPU (its semantics sum every RANK's copy in rank order)
    if (d->variant == ALLRED_MEM && d->local_ranks > 1) return ALLRED_ERR_UNSUPPORTED;
    const size_t n = (size_t)d->elems;
    if (n == 0 || n % 8) return ALLRED_ERR_ARG;
    if (d->variant != ALLRED_LO && n % (8 * (size_t)d->total_nodes)) return ALLRED_ERR_ARG;
    if (d->local_ranks > 1 && (d->local_ranks & (d->local_ranks - 1))) return ALLRED_ERR_ARG;
    return build_schedule(d->algo, d->side_length, d->total_nodes, s, nullptr);
}

size_t partial_bytes(const allred_dist_desc* d) { return d->local_ranks > 1 ? (size_t)d->elems * 2 : 0; }

// ---------------- host twin helpers ----------------
void host_add(uint16_t* dst, const uint16_t* src, size_t n) {
    for (size_t i = 0; i < n; ++i)
        dst[i] = bf16_from_float_rne(bf16_to_float(dst[i]) + bf16_to_float(src[i]));
}

// tree reduce over L local ranks in schedule tree order, bf16 rounding per level
void host_tree_reduce(const uint16_t* ranks, size_t stride, size_t n, const allred_schedule& s, uint16_t* out) {
    const int L = s.total;
    std::vector<uint16_t> v((size_t)L);
    for (size_t e = 0; e < n; ++e) {
        for (int i = 0; i < L; ++i) v[i] = ranks[(size_t)s.tree_order[0][i] * stride + e];
        for (int w = 1; w < L; w *= 2)
            for (int i = 0; i < L; i += 2 * w)
                v[i] = bf16_from_float_rne(bf16_to_float(v[i]) + bf16_to_float(v[i + w]));
        out[e] = v[0];
    }
}

// device copy of the tree order of a (algo, side, total) schedule, cached for the process.  Its callers
// reduce tree 0 (row 0); all `total` rows are there because the persistent one-row kernel
// (k_tree_lds_pipe<P, false>) stages the P rows of the table whichever row it then uses
std::mutex g_order_mu;
std::map<std::tuple<int, int, int, int>, uint8_t*> g_orders;

int device_order(int algo, int side, int total, const uint8_t** out) {
    int dev = 0;
    (void)hipGetDevice(&dev);
    std::lock_guard<std::mutex> g(g_order_mu);
    auto key = std::make_tuple(dev, algo, side, total);
    auto it = g_orders.find(key);
    if (it == g_orders.end()) {
        allred_schedule s;
        int st = build_schedule(algo, side, total, &s, nullptr);
        if (st != ALLRED_OK) return st;
        uint8_t* p = nullptr;
        const size_t bytes = (size_t)s.total * ALLRED_MAX_NODES;
        if (hipMalloc((void**)&p, bytes) != hipSuccess) return ALLRED_ERR_NOMEM;
        if (hipMemcpy(p, s.tree_order[0], bytes, hipMemcpyHostToDevice) != hipSuccess) return ALLRED_ERR_HIP;
        it = g_orders.emplace(key, p).first;
    }
    *out = it->second;
    return ALLRED_OK;
}

// ---- mem_2D across ranks (allred_mem_2D.cpp:4-165, local_ranks == 1) ----------
// Every rank sends its copy of block q to rank q and receives every rank's copy
// of its own block (pairwise rounds: round k pairs rank r with r ^ k, a perfect
// matching per round, all links at once on the full mesh); the owner sums them in
// mem_2D order — its own copy first, then ranks 0 .. N-1 — in fp32 rounded once
// (or bf16 per add, ALLRED_ACC_BF16: the reference's dest register), then every
// block goes back to every rank.  Staging row 0 = the own copy, row 1 + i = the
// i-th other rank in ascending order.
int mem_row(int q, int me) { return q == me ? 0 : (q < me ? q + 1 : q); }

void host_rows_sum(const uint16_t* rows, size_t stride, size_t n, int nrows, bool acc16, uint16_t* dst) {
    for (size_t e = 0; e < n; ++e) {
        float a = bf16_to_float(rows[e]);
        for (int r = 1; r < nrows; ++r) {
            a += bf16_to_float(rows[(size_t)r * stride + e]);
            if (acc16) a = bf16_to_float(bf16_from_float_rne(a));
        }
        dst[e] = bf16_from_float_rne(a);
    }
}

int run_program(allred_comm* c, const allred_dist_desc* d, const allred_schedule& s, uint16_t* bucket,
                uint16_t* staging, void* stream, Part part = kWhole);

// ---- bounded RCCL ----------------------------------------------------------
// The reference's host blocks in Finish() forever when a core never signals
// (allred_helper.hpp:84-96).  Here every RCCL wait has a deadline: the
// communicator is non-blocking, its pending state is polled, and past the
// deadline it is aborted (ncclCommAbort makes its kernels leave their waits).
// Fault injection (tune "rccl_fault", a bit mask) keeps a wait pending as if
// a peer never arrived, so the abort path is testable on one GPU.
enum class Fault : int64_t { none = 0, init = 1, group = 2, drain = 4 };

int env_timeout_ms() {
    static const int v = [] {
        const char* e = std::getenv("ALLRED_RCCL_TIMEOUT_MS");
        const long x = e ? std::strtol(e, nullptr, 10) : 0;
        return x > 0 && x < (1l << 30) ? (int)x : 4000;   // the peer kernels' spin bound
    }();
    return v;
}
int op_timeout_ms(const allred_comm* c) { return c->timeout_ms > 0 ? c->timeout_ms : env_timeout_ms(); }
// a node's first RCCL init (topology discovery, connection setup) takes seconds:
// ALLRED_RCCL_INIT_TIMEOUT_MS, default 60 s (never below the operation deadline)
int init_timeout_ms(const allred_comm* c) {
    static const int init = [] {
        const char* e = std::getenv("ALLRED_RCCL_INIT_TIMEOUT_MS");
        const long x = e ? std::strtol(e, nullptr, 10) : 0;
        return x > 0 && x < (1l << 30) ? (int)x : 60000;
    }();
    const int t = op_timeout_ms(c);
    return (tune(Tune::rccl_fault) & (int64_t)Fault::init) ? t : std::max(t, init);
}

void abort_comm(allred_comm* c, hipStream_t hs) {
    if (c->aborted) return;
    if (c->comm) (void)ncclCommAbort(c->comm);
    c->aborted = true;
    c->comm = nullptr;
    if (hs) {   // the aborted kernels drain; bounded, the caller returns an error either way
        const auto t0 = std::chrono::steady_clock::now();
        while (hipStreamQuery(hs) == hipErrorNotReady &&
               std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(op_timeout_ms(c)))
            std::this_thread::sleep_for(std::chrono::microseconds(100));
    }
}

// poll the communicator out of ncclInProgress (non-blocking init / group end / finalize)
int settle(allred_comm* c, int timeout_ms, Fault f) {
    const bool fault = f != Fault::none && (tune(Tune::rccl_fault) & (int64_t)f) != 0;
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        ncclResult_t a = ncclInProgress;
        if (ncclCommGetAsyncError(c->comm, &a) != ncclSuccess) a = ncclInternalError;
        if (fault) a = ncclInProgress;
        if (a == ncclSuccess) return ALLRED_OK;
        if (a != ncclInProgress) {
            abort_comm(c, nullptr);
            return ALLRED_ERR_RCCL;
        }
        if ((c->cancel && c->cancel->load()) ||
            std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(timeout_ms)) {
            abort_comm(c, nullptr);
            return ALLRED_ERR_TRANSPORT;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
}

// after ncclGroupEnd on a non-blocking communicator.  peers: the group's partners
// (bit mask): a group with a partner this communicator never exchanged with
// sets the connection up (seconds on a busy node) and gets the init deadline
int group_end(allred_comm* c, bool ok, uint64_t peers) {
    const ncclResult_t r = ncclGroupEnd();
    if (!ok || (r != ncclSuccess && r != ncclInProgress)) return ALLRED_ERR_RCCL;
    int st = ALLRED_OK;
    if (r != ncclSuccess || (tune(Tune::rccl_fault) & (int64_t)Fault::group))
        st = settle(c, (peers & ~c->connected) ? init_timeout_ms(c) : op_timeout_ms(c), Fault::group);
    if (st == ALLRED_OK) c->connected |= peers;
    return st;
}

}  // namespace

namespace tsa {

int local_tree_order(int algo, int side, int total, const uint8_t** out) { return device_order(algo, side, total, out); }

int dist_check_desc(const allred_dist_desc* d, allred_schedule* s) { return check_desc(d, s); }

void comm_set_cancel(allred_comm* c, const std::atomic<int>* cancel) {
    if (c) c->cancel = cancel;
}

// The RCCL program's exchanges, as tables for the peer-mapped kernel
// (k_peer_sched): per channel, the step partner and this rank's block masks
// in the channel's labels, plus the channel slice in 16-byte vectors.
int peer_prog(const allred_dist_desc* d, int rank, PeerProg* out) {
    allred_schedule s;
    int st = check_desc(d, &s);
    if (st != ALLRED_OK) return st;
    if (rank < 0 || rank >= d->total_nodes || s.steps > kPeerMaxSteps) return ALLRED_ERR_ARG;
    const size_t n = (size_t)d->elems;
    const int N = s.total, S = s.steps;
    int C = channels_for(s, d->channels, n);
    if (d->variant == ALLRED_LO && n % (8 * (size_t)N)) C = 1;
    if (C > kPeerMaxChannels) C = kPeerMaxChannels;
    *out = PeerProg{};
    out->S = S;
    out->C = C;
    out->N = N;
    out->lo = d->variant == ALLRED_LO;
    auto id_of = [&](int c, int r) { return C == 1 ? r : gf_mul(gf_pow_alpha(c, S), r, S); };
    for (int c = 0; c < C; ++c) {
        size_t base = 0, len = n;
        if (C > 1) slice_of(n, N, C, c, &base, &len);
        out->base[c] = base / 8;
        out->len[c] = len / 8;
        const int x = id_of(c, rank);
        for (int k = 0; k < S; ++k) {
            const int px = s.partner[x][k];
            int q = px;
            if (C > 1)
                for (q = 0; q < N && id_of(c, q) != px; ++q) {}
            out->peer[c][k] = q;
            out->recv[c][k] = s.recv[x][k];
            out->send[c][k] = s.send[x][k];
        }
    }
    return ALLRED_OK;
}

}  // namespace tsa

extern "C" {

int allred_tree_reduce(const uint16_t* ranks, uint64_t stride, size_t n, int algo, int side, int total,
                       uint16_t* out, void* stream) {
    if (!ranks || !out || stride < n) return ALLRED_ERR_ARG;
    const uint8_t* order = nullptr;
    int st = device_order(algo, side, total, &order);
    if (st != ALLRED_OK) return st;
    return launch_tree_reduce(ranks, stride, n, total, order, out, stream);
}

int allred_broadcast(uint16_t* ranks, uint64_t stride, size_t n, int total, const uint16_t* src, void* stream) {
    if (!ranks || !src || stride < n || total < 1) return ALLRED_ERR_ARG;
    return launch_broadcast(ranks, stride, n, total, src, stream);
}

int allred_comm_get_unique_id(uint8_t* id) {
    if (!id) return ALLRED_ERR_ARG;
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return ALLRED_ERR_RCCL;
    std::memcpy(id, &u, sizeof(u));
    return ALLRED_OK;
}

int allred_comm_init(const uint8_t* id, int nranks, int rank, int device, allred_comm** out) {
    if (!id || !out || nranks < 1 || rank < 0 || rank >= nranks) return ALLRED_ERR_ARG;
    *out = nullptr;
    if (device >= 0 && hipSetDevice(device) != hipSuccess) return ALLRED_ERR_HIP;
    auto* c = new allred_comm();
    c->nranks = nranks;
    c->rank = rank;
    (void)hipGetDevice(&c->device);
    ncclUniqueId u;
    std::memcpy(&u, id, sizeof(u));
    ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
    cfg.blocking = 0;
    const ncclResult_t r = ncclCommInitRankConfig(&c->comm, nranks, u, rank, &cfg);
    int st = (r == ncclSuccess || r == ncclInProgress) ? settle(c, init_timeout_ms(c), Fault::init) : ALLRED_ERR_RCCL;
    if (st != ALLRED_OK) {   // a rank that never joins: aborted past the deadline, no hang
        if (c->comm && !c->aborted) (void)ncclCommAbort(c->comm);
        delete c;
        return st;
    }
    *out = c;
    return ALLRED_OK;
}

int allred_comm_init_all(int ndev, const int* devices, allred_comm** out) {
    if (!devices || !out || ndev < 1 || ndev > ALLRED_MAX_NODES) return ALLRED_ERR_ARG;
    for (int i = 0; i < ndev; ++i) out[i] = nullptr;
    // ncclCommInitAll's work as one group of non-blocking ncclCommInitRankConfig
    // calls (one unique id, rank i on devices[i]), so init is bounded too
    ncclUniqueId u;
    if (ncclGetUniqueId(&u) != ncclSuccess) return ALLRED_ERR_RCCL;
    std::vector<allred_comm*> cs((size_t)ndev, nullptr);
    for (int i = 0; i < ndev; ++i) {
        cs[(size_t)i] = new allred_comm();
        cs[(size_t)i]->nranks = ndev;
        cs[(size_t)i]->rank = i;
        cs[(size_t)i]->device = devices[i];
    }
    int st = ALLRED_OK;
    int prev_dev = 0;   // the caller's current device, restored below (ncclCommInitAll leaves it alone)
    if (hipGetDevice(&prev_dev) != hipSuccess) prev_dev = -1;
    if (ncclGroupStart() != ncclSuccess) st = ALLRED_ERR_RCCL;
    for (int i = 0; i < ndev && st == ALLRED_OK; ++i) {
        ncclConfig_t cfg = NCCL_CONFIG_INITIALIZER;
        cfg.blocking = 0;
        if (hipSetDevice(devices[i]) != hipSuccess) { st = ALLRED_ERR_HIP; break; }
        const ncclResult_t r = ncclCommInitRankConfig(&cs[(size_t)i]->comm, ndev, u, i, &cfg);
        if (r != ncclSuccess && r != ncclInProgress) st = ALLRED_ERR_RCCL;
    }
    const ncclResult_t ge = ncclGroupEnd();
    if (prev_dev >= 0) (void)hipSetDevice(prev_dev);
    if (st == ALLRED_OK && ge != ncclSuccess && ge != ncclInProgress) st = ALLRED_ERR_RCCL;
    for (int i = 0; i < ndev && st == ALLRED_OK; ++i) st = settle(cs[(size_t)i], init_timeout_ms(cs[(size_t)i]), Fault::init);
    if (st != ALLRED_OK) {
        for (allred_comm* c : cs) {
            if (c->comm && !c->aborted) (void)ncclCommAbort(c->comm);
            delete c;
        }
        return st;
    }
    for (int i = 0; i < ndev; ++i) out[i] = cs[(size_t)i];
    return ALLRED_OK;
}

int allred_comm_destroy(allred_comm* c) {
    if (!c) return ALLRED_OK;
    if (c->comm && !c->aborted) {
        // non-blocking teardown: finalize (polled against the deadline), then destroy;
        // a finalize that never settles is aborted instead
        const ncclResult_t f = ncclCommFinalize(c->comm);
        const int st = (f == ncclSuccess || f == ncclInProgress) ? settle(c, op_timeout_ms(c), Fault::none) : ALLRED_ERR_RCCL;
        if (st == ALLRED_OK) (void)ncclCommDestroy(c->comm);
        else if (!c->aborted) (void)ncclCommAbort(c->comm);
    }
    delete c;
    return ALLRED_OK;
}

int allred_comm_set_timeout(allred_comm* c, int timeout_ms) {
    if (!c || timeout_ms < 0) return ALLRED_ERR_ARG;
    c->timeout_ms = timeout_ms;
    return ALLRED_OK;
}

int allred_comm_wait(allred_comm* c, void* stream) {
    if (!c) return ALLRED_ERR_ARG;
    if (c->aborted) return ALLRED_ERR_TRANSPORT;
    hipStream_t hs = (hipStream_t)stream;
    const auto t0 = std::chrono::steady_clock::now();
    const auto limit = std::chrono::milliseconds(op_timeout_ms(c));
    const bool fault = (tune(Tune::rccl_fault) & (int64_t)Fault::drain) != 0;
    for (;;) {
        const hipError_t q = hipStreamQuery(hs);
        if (q == hipSuccess && !fault) break;
        if (q != hipSuccess && q != hipErrorNotReady) return ALLRED_ERR_HIP;
        ncclResult_t a = ncclSuccess;
        if (c->comm && ncclCommGetAsyncError(c->comm, &a) == ncclSuccess && a != ncclSuccess && a != ncclInProgress) {
            abort_comm(c, hs);
            return ALLRED_ERR_RCCL;
        }
        if ((c->cancel && c->cancel->load()) || std::chrono::steady_clock::now() - t0 > limit) {
            abort_comm(c, hs);   // its kernels leave their waits; the stream drains (bounded)
            return ALLRED_ERR_TRANSPORT;
        }
        std::this_thread::sleep_for(std::chrono::microseconds(20));
    }
    return ALLRED_OK;
}

int allred_comm_aborted(const allred_comm* c) { return c && c->aborted ? 1 : 0; }

size_t allred_dist_workspace_bytes(const allred_dist_desc* d) {
    if (!d) return 0;
    return (size_t)d->elems * 2 + partial_bytes(d);
}

int allred_dist_allreduce(allred_comm* c, const allred_dist_desc* d, uint16_t* buf, void* workspace,
                          void* stream) {
    if (!c || !buf || !workspace) return ALLRED_ERR_ARG;
    if (c->aborted) return ALLRED_ERR_TRANSPORT;
    // a pipelined bucket is pending: its partial lives in [ws, ws + 2n) that this
    // call would overwrite (flush the sequence first, as the peer path demands)
    if (c->pend) return ALLRED_ERR_ARG;
    allred_schedule s;
    int st = check_desc(d, &s);
    if (st != ALLRED_OK) return st;
    if (d->total_nodes != c->nranks) return ALLRED_ERR_ARG;
    // the step adds (k_add_segs) take 16-byte aligned buckets: refuse before the
    // first exchange, never between two RCCL groups (the partners would be left
    // waiting in a step this rank never enters)
    if (((uintptr_t)buf | (uintptr_t)workspace) % 16) return ALLRED_ERR_ARG;
    hipStream_t hs = (hipStream_t)stream;
    const size_t n = (size_t)d->elems;
    uint16_t* staging = static_cast<uint16_t*>(workspace);
    uint16_t* bucket = buf;
    if (d->variant == ALLRED_MEM) {
        const int N = c->nranks, me = c->rank;
        const size_t blk = n / (size_t)N;
        uint16_t* own = buf + (size_t)me * blk;
        if (hipMemcpyAsync(staging, own, blk * 2, hipMemcpyDeviceToDevice, hs) != hipSuccess) return ALLRED_ERR_HIP;
        for (int phase = 0; phase < 2; ++phase) {   // 0: copies of block q to owner q; 1: the sums back
            if (N == 1) break;
            if (ncclGroupStart() != ncclSuccess) return ALLRED_ERR_RCCL;
            bool ok = true;
            for (int k = 1; k < N; ++k) {
                const int q = me ^ k;
                const uint16_t* snd = phase == 0 ? buf + (size_t)q * blk : own;
                uint16_t* rcv = phase == 0 ? staging + (size_t)mem_row(q, me) * blk : buf + (size_t)q * blk;
                ok = ok && ncclSend(snd, blk * 2, ncclUint8, q, c->comm, hs) == ncclSuccess;
                ok = ok && ncclRecv(rcv, blk * 2, ncclUint8, q, c->comm, hs) == ncclSuccess;
            }
            uint64_t peers = 0;
            for (int k = 1; k < N; ++k) peers |= 1ull << (me ^ k);
            if ((st = group_end(c, ok, peers)) != ALLRED_OK) return st;
            if (phase == 0) {
                st = launch_rows_sum(staging, blk, blk, N, own, d->mem_accum == ALLRED_ACC_BF16, stream);
                if (st != ALLRED_OK) return st;
            }
        }
        return ALLRED_OK;
    }
    if (d->local_ranks > 1) {
        // the GPU's partial: the two halves of the workspace swap the partial / staging
        // roles on every call.  A partial rewritten in the same place by consecutive
        // steps made the following broadcast run 13.6 instead of 8 us (rows just read
        // by the tree; tools/bcast_probe.py, profiles/r03_bcast_probe.txt)
        if (c->calls++ & 1) {
            bucket = staging;
            staging += n;
        } else {
            bucket = staging + n;
        }
        st = allred_tree_reduce(buf, n, n, d->local_algo, d->local_side, d->local_ranks, bucket, stream);
        if (st != ALLRED_OK) return st;
    }
    st = run_program(c, d, s, bucket, staging, stream);
    if (st == ALLRED_OK && d->local_ranks > 1) st = launch_broadcast(buf, n, n, d->local_ranks, bucket, stream);
    return st;
}

int allred_dist_allreduce_pipelined(allred_comm* c, const allred_dist_desc* d, uint16_t* cur, void* workspace,
                                    void* stream) {
    if (!c || !d || !workspace) return ALLRED_ERR_ARG;
    if (c->aborted) return ALLRED_ERR_TRANSPORT;
    if (!cur) {   // flush: the pending bucket's rows from its allreduced partial
        if (!c->pend) return ALLRED_ERR_ARG;
        const int st = launch_broadcast(c->pend, c->pend_elems, c->pend_elems, c->pend_local, c->pend_partial, stream);
        c->pend = nullptr;
        return st;
    }
    allred_schedule s;
    int st = check_desc(d, &s);
    if (st != ALLRED_OK) return st;
    if (d->total_nodes != c->nranks || d->local_ranks < 2 || d->variant == ALLRED_MEM) return ALLRED_ERR_ARG;
    if (((uintptr_t)cur | (uintptr_t)workspace) % 16) return ALLRED_ERR_ARG;
    const size_t n = (size_t)d->elems;
    if (c->pend && (n != c->pend_elems || d->local_ranks != c->pend_local)) return ALLRED_ERR_ARG;
    // cur's rows are read while the pending bucket's are written (k_tree_bcast_x, __restrict__):
    // the two buckets must not overlap
    if (c->pend) {
        const size_t span = (size_t)d->local_ranks * n;
        if (cur < c->pend + span && c->pend < cur + span) return ALLRED_ERR_ARG;
    }
    // two parities of [staging n | partial n]: the pending bucket's partial survives this call
    const int parity = c->pend ? c->pend_parity ^ 1 : 0;
    uint16_t* staging = static_cast<uint16_t*>(workspace) + (size_t)parity * 2 * n;
    uint16_t* partial = staging + n;
    const uint8_t* order = nullptr;
    if ((st = local_tree_order(d->local_algo, d->local_side, d->local_ranks, &order)) != ALLRED_OK) return st;
    st = c->pend ? launch_tree_bcast_x(cur, c->pend, n, n, d->local_ranks, order, partial, c->pend_partial, stream)
                 : launch_tree_reduce(cur, n, n, d->local_ranks, order, partial, stream);
    if (st != ALLRED_OK) return st;
    c->pend = cur;   // from here on the bucket is started: its rows are written by the next call or the flush
    c->pend_partial = partial;
    c->pend_parity = parity;
    c->pend_elems = n;
    c->pend_local = d->local_ranks;
    return run_program(c, d, s, partial, staging, stream);
}

int allred_tree_broadcast_pipelined(uint16_t* cur, uint16_t* prev, uint64_t stride, size_t n, int algo, int side,
                                    int total, uint16_t* cur_out, const uint16_t* prev_src, void* stream) {
    if (!cur || !prev || !cur_out || !prev_src || stride < n) return ALLRED_ERR_ARG;
    const uint8_t* order = nullptr;
    int st = device_order(algo, side, total, &order);
    if (st != ALLRED_OK) return st;
    return launch_tree_bcast_x(cur, prev, stride, n, total, order, cur_out, prev_src, stream);
}

}  // extern "C"

namespace {

// the exchange steps of the rank's program on `bucket` (reduce-scatter adds staged in
// `staging`), after the local tree; the caller broadcasts.  part: the whole program, or the
// slice of the cached vector that is its reduce-scatter / all-gather half
int run_program(allred_comm* c, const allred_dist_desc* d, const allred_schedule& s, uint16_t* bucket,
                uint16_t* staging, void* stream, Part part) {
    hipStream_t hs = (hipStream_t)stream;
    const size_t n = (size_t)d->elems;
    int st = ALLRED_OK;
    const int C = channels_for(s, d->channels, n);
    const auto prog = cached_program(d, s, c->rank, C);
    const bool check = tune(Tune::check) != 0;
    if (check && (st = verify_program(d, s, c->rank, C, part)) != ALLRED_OK) return st;
    size_t first, last;
    part_range(part, prog->size(), &first, &last);
    for (size_t q = first; q < last; ++q) {
        const Step& step = (*prog)[q];
        if (check)   // poison every receive region of the step (stream-ordered before the group)
            for (const Exch& e : step.ex)
                for (const Seg& g : e.recv)
                    if (hipMemsetD16Async((hipDeviceptr_t)((e.recv_to_bucket ? bucket : staging) + g.off), kPoison, g.len,
                                          hs) != hipSuccess)
                        return ALLRED_ERR_HIP;
        if (ncclGroupStart() != ncclSuccess) return ALLRED_ERR_RCCL;
        bool ok = true;
        for (const Exch& e : step.ex) {
            for (const Seg& g : e.send)
                ok = ok && ncclSend(bucket + g.off, g.len * 2, ncclUint8, e.peer, c->comm, hs) == ncclSuccess;
            for (const Seg& g : e.recv)
                ok = ok && ncclRecv((e.recv_to_bucket ? bucket : staging) + g.off, g.len * 2, ncclUint8, e.peer,
                                    c->comm, hs) == ncclSuccess;
        }
        // the group is always closed, also after a failed send / recv, so the
        // next call does not start inside a dangling group; a group that never
        // completes (a partner that never arrives) is aborted at the deadline
        uint64_t peers = 0;
        for (const Exch& e : step.ex) peers |= 1ull << e.peer;
        if ((st = group_end(c, ok, peers)) != ALLRED_OK) return st;
        for (size_t i = 0; i < step.add_off.size(); i += kMaxAddSegs) {   // one launch per step (<= 64 segments)
            const int ns = (int)std::min<size_t>(kMaxAddSegs, step.add_off.size() - i);
            st = launch_bf16_add_segs(bucket, staging, step.add_off.data() + i, step.add_len.data() + i, ns, stream);
            if (st != ALLRED_OK) return st;
        }
    }
    return ALLRED_OK;
}

// run_program's host twin: the same slice of the same cached program, exchanges by callback
int run_program_host(const allred_dist_desc* d, const allred_schedule& s, int rank, uint16_t* bucket,
                     uint16_t* scratch, allred_exchange_fn exchange, void* ctx, Part part) {
    int st = ALLRED_OK;
    const int C = channels_for(s, d->channels, (size_t)d->elems);
    const auto prog = cached_program(d, s, rank, C);
    const bool check = tune(Tune::check) != 0;
    if (check && (st = verify_program(d, s, rank, C, part)) != ALLRED_OK) return st;
    std::vector<allred_seg> snd, rcv;
    size_t first, last;
    part_range(part, prog->size(), &first, &last);
    for (size_t q = first; q < last; ++q) {
        const Step& step = (*prog)[q];
        for (const Exch& e : step.ex) {  // channels in order: every channel is a perfect matching
            snd.clear();
            rcv.clear();
            for (const Seg& g : e.send) snd.push_back(allred_seg{bucket + g.off, g.len * 2});
            for (const Seg& g : e.recv) {
                uint16_t* at = (e.recv_to_bucket ? bucket : scratch) + g.off;
                if (check) std::fill(at, at + g.len, kPoison);
                rcv.push_back(allred_seg{at, g.len * 2});
            }
            if (exchange(ctx, e.peer, (int)snd.size(), snd.data(), (int)rcv.size(), rcv.data()) != 0)
                return ALLRED_ERR_TRANSPORT;
        }
        for (size_t i = 0; i < step.add_off.size(); ++i)   // the device path's one add launch per step
            host_add(bucket + step.add_off[i], scratch + step.add_off[i], step.add_len[i]);
    }
    return ALLRED_OK;
}

// what the half-program entry points refuse (before any exchange): anything but a flat,
// one-channel BO desc.  With link-spreading channels the block a rank owns differs per channel.
int half_check_desc(const allred_dist_desc* d, allred_schedule* s) {
    if (!d) return ALLRED_ERR_ARG;
    if (d->variant != ALLRED_BO || d->local_ranks > 1 || d->channels > 1) return ALLRED_ERR_UNSUPPORTED;
    return check_desc(d, s);
}

// channels 0 (auto) would spread a large bucket over the links: the halves run the plain schedule
allred_dist_desc plain_desc(const allred_dist_desc* d) {
    allred_dist_desc p = *d;
    p.channels = 1;
    p.local_ranks = 1;
    return p;
}

int dist_half(allred_comm* c, const allred_dist_desc* d, uint16_t* buf, void* workspace, void* stream, Part part) {
    if (!c || !buf || !workspace) return ALLRED_ERR_ARG;
    if (c->aborted) return ALLRED_ERR_TRANSPORT;
    if (c->pend) return ALLRED_ERR_ARG;   // a pipelined bucket's partial lives in the workspace
    allred_schedule s;
    int st = half_check_desc(d, &s);
    if (st != ALLRED_OK) return st;
    if (d->total_nodes != c->nranks) return ALLRED_ERR_ARG;
    if (((uintptr_t)buf | (uintptr_t)workspace) % 16) return ALLRED_ERR_ARG;
    const allred_dist_desc pd = plain_desc(d);
    return run_program(c, &pd, s, buf, static_cast<uint16_t*>(workspace), stream, part);
}

int dist_half_host(const allred_dist_desc* d, int rank, uint16_t* buf, uint16_t* scratch, allred_exchange_fn exchange,
                   void* ctx, Part part) {
    if (!buf || !scratch || !exchange) return ALLRED_ERR_ARG;
    allred_schedule s;
    int st = half_check_desc(d, &s);
    if (st != ALLRED_OK) return st;
    if (rank < 0 || rank >= d->total_nodes) return ALLRED_ERR_ARG;
    const allred_dist_desc pd = plain_desc(d);
    return run_program_host(&pd, s, rank, buf, scratch, exchange, ctx, part);
}

}  // namespace

extern "C" {

int allred_dist_reduce_scatter(allred_comm* c, const allred_dist_desc* d, uint16_t* buf, void* workspace,
                               void* stream) {
    return dist_half(c, d, buf, workspace, stream, kReduceScatter);
}

int allred_dist_all_gather(allred_comm* c, const allred_dist_desc* d, uint16_t* buf, void* workspace, void* stream) {
    return dist_half(c, d, buf, workspace, stream, kAllGather);
}

int allred_dist_reduce_scatter_host(const allred_dist_desc* d, int rank, uint16_t* buf, uint16_t* scratch,
                                    allred_exchange_fn exchange, void* ctx) {
    return dist_half_host(d, rank, buf, scratch, exchange, ctx, kReduceScatter);
}

int allred_dist_all_gather_host(const allred_dist_desc* d, int rank, uint16_t* buf, uint16_t* scratch,
                                allred_exchange_fn exchange, void* ctx) {
    return dist_half_host(d, rank, buf, scratch, exchange, ctx, kAllGather);
}

int allred_dist_program_stats(const allred_dist_desc* d, int rank, int* steps, int* launches, int* segments) {
    allred_schedule s;
    int st = check_desc(d, &s);
    if (st != ALLRED_OK) return st;
    if (rank < 0 || rank >= d->total_nodes) return ALLRED_ERR_ARG;
    if (d->variant == ALLRED_MEM) {   // one all-to-all group, one ordered sum, one all-gather group
        const int N = d->total_nodes;
        if (steps) *steps = N > 1 ? 2 : 0;
        if (launches) *launches = N > 1 ? 1 : 0;   // one rank: no exchange, no sum kernel
        if (segments) *segments = 4 * (N - 1);
        return ALLRED_OK;
    }
    const auto prog = cached_program(d, s, rank, channels_for(s, d->channels, (size_t)d->elems));
    int k = 0, l = 0, g = 0;
    for (const Step& step : *prog) {
        ++k;
        l += add_launches(step);
        for (const Exch& e : step.ex) g += (int)(e.send.size() + e.recv.size());
    }
    if (steps) *steps = k;
    if (launches) *launches = l;
    if (segments) *segments = g;
    return ALLRED_OK;
}

int allred_dist_allreduce_host(const allred_dist_desc* d, int rank, uint16_t* buf, uint16_t* scratch,
                               allred_exchange_fn exchange, void* ctx) {
    if (!buf || !scratch || !exchange) return ALLRED_ERR_ARG;
    allred_schedule s;
    int st = check_desc(d, &s);
    if (st != ALLRED_OK) return st;
    if (rank < 0 || rank >= d->total_nodes) return ALLRED_ERR_ARG;
    const size_t n = (size_t)d->elems;
    uint16_t* bucket = buf;
    if (d->variant == ALLRED_MEM) {   // the device path's rounds, pair by pair (r ^ k)
        const int N = d->total_nodes;
        const size_t blk = n / (size_t)N;
        uint16_t* own = buf + (size_t)rank * blk;
        std::memcpy(scratch, own, blk * 2);
        for (int k = 1; k < N; ++k) {
            const int q = rank ^ k;
            allred_seg snd{buf + (size_t)q * blk, blk * 2}, rcv{scratch + (size_t)mem_row(q, rank) * blk, blk * 2};
            if (exchange(ctx, q, 1, &snd, 1, &rcv) != 0) return ALLRED_ERR_TRANSPORT;
        }
        host_rows_sum(scratch, blk, blk, N, d->mem_accum == ALLRED_ACC_BF16, own);
        for (int k = 1; k < N; ++k) {
            const int q = rank ^ k;
            allred_seg snd{own, blk * 2}, rcv{buf + (size_t)q * blk, blk * 2};
            if (exchange(ctx, q, 1, &snd, 1, &rcv) != 0) return ALLRED_ERR_TRANSPORT;
        }
        return ALLRED_OK;
    }
    if (d->local_ranks > 1) {
        allred_schedule ls;
        st = build_schedule(d->local_algo, d->local_side, d->local_ranks, &ls, nullptr);
        if (st != ALLRED_OK) return st;
        bucket = scratch + n;
        host_tree_reduce(buf, n, n, ls, bucket);
    }
    if ((st = run_program_host(d, s, rank, bucket, scratch, exchange, ctx, kWhole)) != ALLRED_OK) return st;
    if (d->local_ranks > 1)
        for (int r = 0; r < d->local_ranks; ++r) std::memcpy(buf + (size_t)r * n, bucket, n * 2);
    return ALLRED_OK;
}

}  // extern "C"
