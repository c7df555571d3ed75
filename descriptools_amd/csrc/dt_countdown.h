// dt_countdown.h -- the in-degree countdown on a drainage DAG that D-infinity (dt_dinf.hip, out-degree <= 2) and MFD
// (dt_mfd.hip, out-degree <= 8) accumulate with: the state word, the control words, the workspace, the mark and out
// steps and the host sequence.  What differs between the ops stays in their files: how a cell's in-degree is gathered
// (the init kernel), how a complete cell splits its total and what a lane does with the cells it completes (the flow
// kernel).
//
// One 64-bit word per cell is the whole state,
//   bits 0-55 sum (q, then q + what has arrived) | 56-59 pending donors | 60 source | 61, 62 the op's own flags
// (the pointer doubling of the tile passes carries a tree, not a DAG, so it cannot be used here).
// init   gathers each cell's in-degree from its eight neighbours (no atomics), quantises the weight (cd_quant) and
//        writes the word; a cell without donors is a source.
// flow   a lane that owns a complete cell (pending 0) splits its total T among the receivers and adds m - 2^56 to each
//        receiver's word with one returning 64-bit atomic: sum and countdown move together, the arrival that finds
//        pending == 1 in the value it gets back holds the receiver's complete total, and no fence is needed (the word
//        is the only thing handed over).  That lane carries on from a receiver it completed and keeps the others in LDS;
//        what LDS cannot hold goes on a global queue.  Round 0 starts from the sources (a scan of the raster); every
//        later round drains what the rounds before put on the queue: k_cd_mark moves the window [lo, hi) to the entries
//        written before it ran, and a round whose window is empty returns at once.  A start (a source, a queue entry)
//        completes a bounded number of cells in a round and then queues what it holds: a round lasts as long as its
//        longest walk, and bounded walks keep the rounds short and the queued work moving.  No lane waits for another,
//        and every loop is bounded by its trip count.  A cell is queued only when it is complete and not yet sent on,
//        which happens once: a queue of N entries cannot overflow.  (MFD's mf_enqueue guards the queue store with the
//        queue's length all the same and k_mf_flow clamps its window to it; D-infinity's stores are unguarded.  The
//        asymmetry is known and deliberate for now: the flow kernels are not to change with this header.)
// out    ldexp(T - q, -s) as float64 (cd_result); -100 on nodata and where pending != 0 (on or below a cycle, or -- on
//        the device tier -- not reached within the budget of rounds); tail != hi means queued work is left, which
//        raises DT_STATUS_NOT_CONVERGED (cd_not_converged).
// Integer sums are order-free and the split is a function of the complete T alone, so the result does not depend on
// the order of arrival, on how many cells a lane holds or on the number of rounds.
// Routing (routing.py) puts a transfer function between "complete" and "split": the flow kernels' MODE instances split
// O = cd_transfer(T, the cell's parameter) <= T, the out kernels' take O again from the final word.  The word, the
// control words and the workspace are the accumulation's, whose kernels are the CD_T_NONE instances.
#pragma once
#include <cmath>

#include "dt_kernels.h"

#define CD_SUM_MASK ((1ull << 56) - 1ull)
#define CD_ONE_PEND (1ull << 56)
#define CD_F_SRC (1ull << 60)
#define CD_NONE 0xFFFFFFFFu

// control words of one accumulation: the queue's tail, the window [lo, hi) of the current queue round, queue rounds
// that found work, the largest window, cells with two or more receivers
enum { CD_C_TAIL = 0, CD_C_LO = 1, CD_C_HI = 2, CD_C_ROUNDS = 3, CD_C_HIGH = 4, CD_C_MULTI = 5, CD_C_WORDS = 8 };

// donors of the word's cell that have not arrived yet
__device__ __forceinline__ unsigned long long cd_pending(unsigned long long wv) { return (wv >> 56) & 0xFull; }

// dt_quant_weight of cell c's weight; wt NULL: 1 everywhere
__device__ __forceinline__ unsigned long long cd_quant(const double *__restrict__ wt, long long c, int sbits,
                                                       unsigned long long qmax, bool &bad) {
  return dt_quant_weight(wt ? wt[c] : 1.0, sbits, qmax, bad);
}

// the out kernels, one lane of them (`first`): queued work is left
__device__ __forceinline__ void cd_not_converged(bool first, const uint32_t *__restrict__ ctl,
                                                 int *__restrict__ status) {
  if (first && status && ctl[CD_C_TAIL] != ctl[CD_C_HI]) atomicOr(status, DT_STATUS_NOT_CONVERGED);
}
// the result of a complete cell: what arrived, its own q (cd_quant's, taken again) excluded
__device__ __forceinline__ double cd_result(unsigned long long wv, unsigned long long q, int sbits) {
  return ldexp((double)(long long)((wv & CD_SUM_MASK) - q), -sbits);
}

// ---- routing: a transfer function between "complete" and "split" (routing.py holds the definition) ----
// A complete cell with load T passes on O = f(T, p) <= T and keeps R = T - O; the receivers get the op's split of O.
// The modes are the C ABI's DT_ROUTE_*; CD_T_NONE is the accumulation (O = T, no parameter raster is read).
enum { CD_T_NONE = 0, CD_T_DECAY = DT_ROUTE_DECAY, CD_T_RETAIN = DT_ROUTE_RETAIN, CD_T_LIMIT = DT_ROUTE_LIMIT };
#define CD_CAP_MAX (1ull << 53)  // a capacity is held to this: above every T (<= 2^52), so +inf never binds

// O of a load T < 2^56 under the parameter value p; a p outside its contract is `bad` and acts as the identity
//   decay   D = rint(p * 2^30) in [0, 2^30]: floor(T * D / 2^30), the product split as mf_share splits its own
//   retain  C = min(rint(p * 2^s), 2^53):    T - C above the capacity, else 0
//   limit   the same C:                      min(T, C)
__device__ __forceinline__ unsigned long long cd_transfer_value(int mode, unsigned long long T, double p, int sbits,
                                                                bool &bad) {
  if (mode == CD_T_DECAY) {
    if (!(p >= 0.0 && p <= 1.0)) {
      bad = true;
      return T;
    }
    const unsigned long long D = (unsigned long long)rint(ldexp(p, 30));
    return (T >> 30) * D + (((T & ((1ull << 30) - 1ull)) * D) >> 30);
  }
  if (mode == CD_T_RETAIN || mode == CD_T_LIMIT) {
    if (!(p >= 0.0)) {
      bad = true;
      return T;
    }
    const double c = rint(ldexp(p, sbits));
    const unsigned long long C = c >= (double)CD_CAP_MAX ? CD_CAP_MAX : (unsigned long long)c;
    if (mode == CD_T_RETAIN) return T > C ? T - C : 0ull;
    return T < C ? T : C;
  }
  return T;
}
// the same on the parameter raster: the flow and the out kernels take O of cell c from here (the flow kernels that
// have the value in a register already, loaded ahead of its use, call cd_transfer_value on it)
__device__ __forceinline__ unsigned long long cd_transfer(int mode, unsigned long long T,
                                                          const double *__restrict__ param, long long c, int sbits,
                                                          bool &bad) {
  return mode == CD_T_NONE ? T : cd_transfer_value(mode, T, param[c], sbits, bad);
}

// the four rasters of a routing run, each NULL when it is not wanted: what arrived (T - q), T, O and T - O
struct CdRouteOut {
  double *inflow, *load, *outflow, *retained;
};
// one complete cell of an out kernel: O and R are taken again from the final word and the parameter
__device__ __forceinline__ void cd_route_store(int mode, const CdRouteOut &o, long long c, bool complete,
                                               unsigned long long wv, unsigned long long q,
                                               const double *__restrict__ param, int sbits) {
  double vi = -100.0, vl = -100.0, vo = -100.0, vr = -100.0;
  if (complete) {
    const unsigned long long T = wv & CD_SUM_MASK;
    bool ignore = false;  // the init kernel has reported it
    const unsigned long long O = cd_transfer(mode, T, param, c, sbits, ignore);
    vi = ldexp((double)(long long)(T - q), -sbits);
    vl = ldexp((double)(long long)T, -sbits);
    vo = ldexp((double)(long long)O, -sbits);
    vr = ldexp((double)(long long)(T - O), -sbits);
  }
  if (o.inflow) o.inflow[c] = vi;
  if (o.load) o.load[c] = vl;
  if (o.outflow) o.outflow[c] = vo;
  if (o.retained) o.retained[c] = vr;
}

// the workspace: control words, one word and one queue slot per cell and, with `edges`, one byte per cell
struct CdLayout {
  uint32_t *ctl;
  unsigned long long *word;
  uint32_t *queue;
  uint8_t *edges;
  size_t bytes;
};
static inline CdLayout cd_layout(int64_t N, void *scratch, bool edges) {
  CdLayout L = {};
  DtCarver c(scratch);
  L.ctl = c.take<uint32_t>(CD_C_WORDS);
  L.word = c.take<unsigned long long>((size_t)N);
  L.queue = c.take<uint32_t>((size_t)N);
  if (edges) L.edges = c.take<uint8_t>((size_t)N);
  L.bytes = c.bytes();
  return L;
}

// the largest weight word: N of them sum to at most 2^52
static inline unsigned long long cd_qmax(int64_t N) { return (1ull << 52) / (unsigned long long)N; }
// complete cells a lane holds in LDS beside the one it carries on with: `stack`, or n - 1 with stack_cap = n > 0
static inline int cd_stack_cap(int stack_cap, int stack) {
  return stack_cap > 0 && stack_cap - 1 < stack ? stack_cap - 1 : stack;
}

// k_cd_mark (dt_countdown.hip): the window of the next queue round
void cd_launch_mark(hipStream_t s, uint32_t *ctl);

// start != 0: the control words are cleared, init() and round 0, flow(true, one lane per cell); then `rounds` queue
// rounds, each k_cd_mark and flow(false, a capped grid); finish != 0: out(one lane per cell).  The three launch the
// op's own kernels on `s`.  Nothing synchronises.
template <typename Init, typename Flow, typename Out>
static int cd_run(hipStream_t s, int64_t N, uint32_t *ctl, int start, int rounds, int finish, Init init, Flow flow,
                  Out out) {
  const dim3 cells((unsigned)((N + 255) / 256));
  if (start) {
    DT_HIP(hipMemsetAsync(ctl, 0, sizeof(uint32_t) * CD_C_WORDS, s));
    init();
    flow(true, cells);
  }
  const dim3 gq(dt_capped_grid(N, 2048));
  for (int r = 0; r < rounds; r++) {
    cd_launch_mark(s, ctl);
    flow(false, gq);
  }
  if (finish) out(cells);
  return DT_OK;
}
