// step_deep.hip -- the one-launch accelerated-RGD iteration with the stream taken OFF its critical path ("deep carry",
// round 6).  k_step_fe<R, 0> (step_fused.hip) removed every dependent round trip but one
// from the front of the launch; what was left of its 14.2 us was a chain: cold round trip 3.4 -> the 128 KB slab of
// M = (Q + shift I)^-1 per CU 4.9 -> product 1.1 -> per-pose tail 3.0 -> launch gap 2.2.  The slab is STATIC data and
// 80 % of the vector it meets is known a launch early, so the chain need not contain it:
//
//   * the rows of the gradient of agent c that belong to PRIVATE poses (no shared edge) are the tangent projection of the
//     carried row products -- complete two launches before c's turn (B_CARRY_G, formed from the evaluation point the
//     look-ahead wave left three launches before).  Only the public poses (the first and last 50 of a 500-pose agent of
//     sphere2500 / 5) need the neighbours' poses of the launch before.
//   * a column of the product  z[col] = sum_k M[k, col] g[k]  is accumulated by 32 lanes, lane kl taking rows
//     2 kl + 64 m (+ 1) for m = 0 .. 31 in one fixed order of the 64-row chunks m: the agent's chunk order (AgentDev::fe_ord,
//     private chunks first; k_precond follows the same order).  The first M0 chunks of every agent are private.  So launch
//     k - 1 streams those M0 chunks of M_c against the carried gradient and leaves the 256 x R partial sums of every
//     workgroup (PACC); launch k loads them and continues the SAME chain of fused multiply-adds over the remaining
//     32 - M0 chunks: bitwise the sums k_precond forms in one go.
//
// Launch k (agent c = sel(k); d = sel(k+1), e = sel(k+2), f = sel(k+3); four different agents in a row):
//     IN  finish the gradient of c's public poses, continue PACC(c) over the last 32 - M0 chunks, step c's poses
//         (tangent projection, QF retraction, Nesterov V, look-ahead Y), look-ahead of everybody else
//     P   stream the M0 private chunks of M_d against carry-G(d): PACC(d)                    (consumed by launch k + 1)
//     W   row products of e at its evaluation point, their tangent projection: carry-W/X/G(e) (k + 1: P, k + 2: IN)
//     Y   the point f will be evaluated at: three look-ahead maps in a row, carry-Y(f)        (k + 1: W)
// A run opens with k_fd_prime (the points of sel(0), sel(1), sel(2)), k_fd_rows (W for sel(0) and sel(1)) and k_fd_partial
// (P for sel(0)): three short launches.
//
// Eight waves, eight roles, ONE workgroup barrier.  A wave that requests the stream stays at the issue of its loads until
// most of them have landed (step_fused.hip), and every s_barrier behind that point waits for it -- the critical chain
// (gradient of the public poses -> product over the last chunks -> tail) must not meet the streamers again.  So the only
// s_barrier stands at the kernel's head (it zeroes the counters); every hand-off is a counter in LDS that only the waves
// concerned wait at -- the first of them (RQ) orders the requests: waves 4-7 count themselves in behind their last load (and
// behind no load's DATA: see "the count-in waits for no data" below), the streamers release the stream when all four have
// (everything the chain needs is in the CU's memory queue in front of it):
//     waves 0-3  streamers: coefficients of the shared edges -> LDS (E: four of its five counts), the carried gradient of c's
//                last chunks -> LDS (C); then the whole P part on their own (N: their own hand-off, signalled with the
//                stream still in flight; they start their product behind F, the chain's -- the two share the LDS -- and
//                follow the chunks as they land)
//     waves 4-5  the chain: one public pose per lane (G_j from LDS, projection; rows -> LDS: D) -> their quarters of the
//                product over the last chunks (F) -> wave 4: reduction, step of the two poses on 16 lanes each
//                (step_two_poses); wave 5: W
//     wave 6     neighbour poses of the shared edges -> LDS (E: the fifth count); its quarter of the product behind D (F);
//                the books
//     wave 7     its quarter of the product (F); look-ahead of the other agents' poses + Y
//   Waves 4-7 run at raised priority while they are on the chain.
// The launch's arguments are a HEAD of thirteen plain dwords (step_head.h: the agent's first work vector, M, the partial
// sums, the packed coefficients, n | npub, nshared | parity | flags, the ids of the last chunks, the workgroup count) and,
// behind it, everything else in one struct (FdArgs: the descriptor, what the launch needs of the next two agents, ...).  The
// head is delivered in SGPRs at wave launch (the object is built with -amdgpu-kernarg-preload-count=14; where the firmware
// does not preload, a prologue the compiler emits fetches the same dwords), FdArgs sits in memory nobody has touched.  So
// every role forms its FIRST requests from the head alone -- the streamers the coefficients and the carried rows; the chain
// waves their public pose's record, W / X, their quarter of the last chunks, the operands of the tail; wave 6 the addresses
// of its edges' neighbour poses, its quarter and, through the addresses, the poses; wave 7 its quarter -- and
// only then calls fd_args_behind_requests: one word of every line of FdArgs touched, all in flight at once, and no load of
// the struct can be moved above that point (where the wait for it would stand in front of those requests: the kernel's one
// barrier, whose LDS write shares the scalar loads' counter, waited for the arguments in every wave).  Nothing in front of
// the barrier reads memory: the workgroup's place in the grid follows from the head too (profiles/r21_step_head.md).
// What a role LOOKS UP before it can ask for data -- where the neighbour pose of each shared edge lives (wave 6), which
// pose, which edges and which place in the chunk order a lane's public pose has (the chain waves) -- does not change from
// launch to launch, so it is not resolved in the launch: the host forms it where it builds the descriptor (assembly.hip) and
// keeps it in a FRONT TABLE behind the packed coefficients, at a fixed offset of the allocation the head's fe_coef points at
// (step_front.h).  Those reads are the roles' first instructions; the descriptor's own copies (fe_code, FeBases, pub_pose,
// pub_ptr) serve k_step_fe, k_precond and the evaluations.  A team whose table is not the one built from the descriptors as
// last published (Agent::front_gen against dpgo_team::desc_gen) does not take this form (fe_deep_m0).
// Where a launch's 12.6 us went in round 6 (profiles/r06_deep_carry.md): 2.8 until everything is requested (134 KB per CU in front of
// the stream -- every workgroup finishes ALL public poses itself, the price of no exchange inside the launch), 1.0 until the
// edges' operands have landed, 1.9 gradient of the public poses, 0.9 product over the last chunks, 0.5 reduction, 3.2 tail,
// 2.2 from the last workgroup's end to the next launch's first instruction.  The stream (128 KB per CU) lands under all
// of it: the streamers are done 3 us before the tail.  With the head the launch takes 11.3 us dispatch to dispatch
// (12.5 without, same session): the first requests of every role moved forward by 0.1-0.2 us only -- a data trip remains --,
// most of the gain is in front of the first instruction and behind the last (r21_step_head.md: stamps of both builds).
// With the front table (profiles/r26_step_front.md; trace build, us from wave 4's first instruction, parent -> table): wave 6
// requests the neighbour poses at 1.2-1.4 (2.6) and hands them over at 2.1-2.2 (3.1-3.2); the chain waves count in at 2.4-2.6
// (2.8-3.2), the stream is released at 2.6-2.8 (3.3-3.4); E, seen by the chain, 3.4-3.7 (3.7-3.8) -- it is wave 7's hand-off
// of the coefficients (3.3-3.6), which stands behind its count-in, and moving it in front (three placements) measured slower;
// D 4.9-5.4 (5.7-5.8); tail end, median over the workgroups, 10.64 (10.80); streamers' end 8.55 (8.63): the stream still lands
// under the chain.  Product builds: 11.43 us dispatch to dispatch against 11.58 for the parent in the same sessions.
// THE COUNT-IN WAITS FOR NO DATA (r27, profiles/r27_count_in.md; held on the assembly by tests/test_step_count_in_build.py).
// vmcnt retires in order: a wait for ANY load of a wave in front of its count-in is a wait for everything it requested before
// that load, the loads of M from HBM among them, and the count-in then stands behind the data, not behind the requests.  The
// parent had such waits in three places, read off its assembly (k = loads issued, vmcnt(n) blocks when n < k; <5, 24>):
//   * the chain waves and wave 7 brought the Nesterov state's `iter` to a scalar register in front of the count-in: vmcnt(1)
//     after 47 loads, vmcnt(20) after 57.  Now fd_nest_request asks for the state in front of the count-in and leaves it in
//     vector registers; fd_nest_state consumes it where it is first used, behind the role's product (directly behind the
//     count-in the same wait stood in front of wave 7's hand-off E, and measured slower than the parent);
//   * wave 7 fetched ybase / npose of its lane's agent with vector loads from the argument segment: vmcnt(2) after 37 loads
//     in front of its first look-ahead address.  Now it selects VALUES among the eight it holds in scalar registers;
//   * the chain waves stalled twice while issuing, on registers of load halves nobody reads (the `pose` word of the front
//     table's record, the translation half of a pair of the point): vmcnt(16) after 17, vmcnt(8) after 25.  Now they request
//     12 bytes of the record and the rotation block of the point only.
// Wave 6 keeps its three counted waits, one in front of the pose loads of each address.  No instance has a flat_ access (one
// is enough for the compiler to turn every counted wait into vmcnt(0)).  Trace build, r27 (parent in the same session): the
// chain waves count in at 2.0-2.2 (2.4-2.8), wave 7 at 2.3-2.4 (2.5-2.8), the stream is released at 2.5-2.6 (2.6-3.0), E is
// seen at 3.4-3.5 (3.4-3.8).  Product builds: 11.13-11.15 us dispatch to dispatch against 11.43-11.44 for the parent.
// THE STREAMERS HAND THE COEFFICIENTS OVER, AND FOLLOW THEIR STREAM CHUNK BY CHUNK (r29, profiles/r29_coef_handoff.md; held on
// the assembly by tests/test_step_coef_handoff_build.py).  The chain held all it needed from about 2.2 us and waited until
// 3.4 for E: wave 7 requested the packed coefficients first but handed them over behind its other 35 requests and its
// count-in, in 20 guarded LDS writes.  The streamers are idle there.  They now request the coefficients as their first
// loads -- five per lane over the 1280 parts, clamped to the last part --, the carried rows behind them, write the
// coefficients behind counted waits that leave the carried rows in flight, and count at E (five counts: wave 6 and the
// four of them); a lane beyond the last part writes the clamped part to its own place, so the stretch has no branch.  Wave
// 7 goes from its count-in straight to D.  Trace build (parent in the same session): E seen at 2.3-2.6 (3.4-3.5), D 3.9-4.3
// (5.0-5.3), tail end, median over the workgroups, 9.47 (10.40) -- and the PRODUCT build did not separate: 11.10-11.16 us
// dispatch to dispatch against 11.13-11.16 in five sessions.  The wave ends of a build that stores nothing else showed the
// streamers leaving WITH the tail wave (0.5-1.8 us before it in the parent): the stream had become as long a path as the
// chain.  What held it, read off the assembly: one load of the next agent's carried rows scheduled in among the 24 loads of
// M and one sunk into its guarded write -- vmcnt(4) and vmcnt(0) in front of the hand-off N, a wait for the whole stream, and
// a product that began behind the last chunk's data.  Now those rows are requested in front of the first load of M
// (sched_barrier) and written unguarded (clamped index): the writes leave the 24 loads in flight and the product waits
// chunk by chunk, vmcnt(23) ... (0), from F on -- which the first change had moved a microsecond forward.  The streamers
// leave 1.0 us earlier (7.4-8.5 against 8.4-9.8), the tail wave decides the launch again.  Product builds, both changes,
// four sessions with the parent interleaved: 10.71-10.77 us dispatch to dispatch against 11.14-11.16 (-0.39 ... -0.45 us),
// bench value 0.01113-0.01121 ms against 0.01156-0.01161 (-3.2 ... -3.9 %); every reading below every reading of the parent
// in all four, for both figures.  r26's second condition (medians apart by more than three times the parent's spread) is
// reached for the kernel in three sessions of the four and for the value in two: a gain by that definition in two
// sessions for both figures, not in the other two.  The first change alone is no gain in any session.
// The chain sees E 0.1 us behind its own count-in, the last of the four: it is not idle for wave 6, whose 30 guarded
// writes were therefore left as they are.
// Same arithmetic on the same operands in the same order as k_step_fe / the two-launch sequence: the iterates are BITWISE
// theirs (tests/test_gpu_fused_step.py, profiles/experiments/fe_fuzz.py).  The Nesterov scalars (nest_ahead), the books
// (step_books), the look-ahead map (lookahead_map) and the step of the two poses (step_two_poses) are the text of
// nesterov_step.h, which k_step_fe calls too: for the scalars, the map and the tail "bitwise the two-launch sequence" holds
// BY CONSTRUCTION; for the gradient and the product it holds by test only.  (Wave 7's look-ahead of the other agents' poses
// keeps its own control flow around the shared map: as a function shared with k_step_fe's second wave it cost this kernel
// 2-4 % more instructions and 0.14 us per launch, profiles/r19_nesterov_step.md.)
#include "kernel_common.h"
#include "step_head.h"
#include "step_front.h"
#include <algorithm>

namespace dpgo {

static_assert(FD_FRONT_EDGES == FE_MAX_EDGES && FD_FRONT_AGENTS == LOOKAHEAD_MAX_AGENTS, "step_front.h repeats these limits");

// ---- device helpers of k_step_fd: hand-offs between the waves of a workgroup through counters in LDS, the chunk-ordered
// layout, the staging of the shared edges' operands, the product over the last chunks
constexpr int FD_KC = 2048;
// build switches of the experiments recorded in profiles/r06_deep_carry.md (every one measured SLOWER than the defaults but
// the last; two more are gone: 16-byte loads per lane of the next agent's slab requested in front of the request hand-off,
// and wave 7 handing the coefficients over before it requested its look-ahead operands -- the streamers hand them over now):
// DPGO_FD_GC_LATE -- the carried rows of the current agent requested behind it; DPGO_FD_PACC_WT -- partial sums stored
// write-through; DPGO_FD_KA_PREFETCH (default on) -- one word of every line of the launch's argument struct touched as soon
// as the requests formed from the head are out (fd_args_behind_requests)
#ifndef DPGO_FD_GC_LATE
#define DPGO_FD_GC_LATE 0
#endif
#ifndef DPGO_FD_PACC_WT
#define DPGO_FD_PACC_WT 0
#endif
#ifndef DPGO_FD_KA_PREFETCH
#define DPGO_FD_KA_PREFETCH 1
#endif

// hand-offs between the waves of the workgroup: counters in LDS (see the head of the file)
enum { FD_SY_C = 0, FD_SY_E, FD_SY_D, FD_SY_F, FD_SY_N, FD_SY_RQ, FD_SY_COUNT = 8 };

__device__ __forceinline__ void fd_signal(int *cnt) {
  // (the LDS operations of one wave execute in order: the count follows the wave's writes)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// the roles that count themselves in at FD_SY_RQ.  Each leaves two comment-only markers in the assembly -- "fd_role_entry k" in
// front of its first request, "fd_count_in k" in front of its count -- which tests/test_step_count_in_build.py walks between
// (FD_ROLE_COEF is wave 7: it handed the coefficients over until r29 and keeps the number the tests know it by.  The
// streamers do not count in at FD_SY_RQ -- they wait for it; their markers are "fd_role_entry 0" and, in front of the count of
// their hand-off E, "fd_e_count 0": tests/test_step_coef_handoff_build.py)
enum { FD_ROLE_STREAM = 0, FD_ROLE_CHAIN = 4, FD_ROLE_POSES = 6, FD_ROLE_COEF = 7 };

template <int ROLE>
__device__ __forceinline__ void fd_role_entry() {
  asm volatile("; fd_role_entry %0" ::"n"(ROLE));
}

// the streamers' hand-off of the coefficients: fd_signal with the marker in front of the count
__device__ __forceinline__ void fd_signal_coef(int *cnt) {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  asm volatile("; fd_e_count %0" ::"n"(FD_ROLE_STREAM) : "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// The Nesterov state of the stepped agent is REQUESTED in front of the count-in and CONSUMED behind it.  Read as a struct it
// is one wave-uniform load whose `iter` the compiler brings to a scalar register at once -- in front of the count-in, behind
// a wait for the load and, since vmcnt retires in order, for everything the wave requested before it (the loads of M from
// HBM among them): the count-in stood behind the data.  So: loaded through a lane-opaque zero offset, the words stay in
// vector registers until fd_nest_state, which the roles call where they first use the state: behind their product.
// (Requesting it behind the count-in is not the same: the load would queue behind the stream.)
struct FdNestReq {
  double gamma, alpha;
  int iter;
};

__device__ __forceinline__ FdNestReq fd_nest_request(const NestState *src) {
  static_assert(offsetof(NestState, gamma) == 0 && offsetof(NestState, alpha) == 8 && offsetof(NestState, iter) == 16, "the words below");
  int z = 0;
  asm volatile("" : "+v"(z));
  const __attribute__((address_space(1))) char *p = (const __attribute__((address_space(1))) char *)src + z;
  FdNestReq rq;
  // (word by word: a word nobody reads behind the count-in is then not requested at all -- the dead half of a wider load is
  // a register the compiler reuses while the load is in flight, behind a wait for it)
  rq.gamma = *(const __attribute__((address_space(1))) double *)p;
  rq.alpha = *(const __attribute__((address_space(1))) double *)(p + 8);
  rq.iter = *(const __attribute__((address_space(1))) int *)(p + 16);
  return rq;
}

__device__ __forceinline__ NestState fd_nest_state(const FdNestReq &rq) {
  NestState ns;
  ns.gamma = rq.gamma; ns.alpha = rq.alpha; ns.iter = __builtin_amdgcn_readfirstlane(rq.iter); ns.pad = 0;
  return ns;
}

// "everything this wave needs is in the CU's memory queue": counted behind the wave's last request (the compiler may move
// neither the requests below it nor the count above them)
template <int ROLE>
__device__ __forceinline__ void fd_signal_requested(int *cnt) {
  __builtin_amdgcn_sched_barrier(0);
  asm volatile("; fd_count_in %0" ::"n"(ROLE) : "memory");
  if ((threadIdx.x & 63) == 0) __hip_atomic_fetch_add(cnt, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  asm volatile("" ::: "memory");
  __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ void fd_wait(int *cnt, int target) {
  // (bounded: the waves of a workgroup are resident together, so the count always arrives -- the bound only keeps a logic
  // error from hanging the device; 4M polls are a fraction of a second)
  for (int spin = 0; spin < (1 << 22) && __hip_atomic_load(cnt, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP) < target; ++spin)
    __builtin_amdgcn_s_sleep(1);
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// where pose p of an agent sits in the chunk-ordered ("position") layout of its vector: chunk p / 16 moves to the place
// it has in the agent's chunk order, [place][16 poses][4r]
template <int R>
__device__ __forceinline__ int fd_pos_off(const unsigned char *ord, int pose) {
  const int ch = pose >> 4;
  int p = 0;
#pragma unroll
  for (int i = 0; i < 32; ++i) p = ((int)ord[i] == ch) ? i : p;
  return p * 64 * R + (pose & 15) * 4 * R;
}

// The operands of the shared edges go to LDS, [edge][neighbour pose 4r | 16 coefficients].
//   * wave 6, neighbour poses: one lane per edge (edges l, 64 + l, 128 + l), 2r loads of 16 bytes each.  Where the neighbour
//     lives is an address the host formed once (step_front.h: xaddr[parity][edge], behind the coefficients) -- three 8-byte
//     loads per lane, the wave's first instructions; k_step_fe forms it in every launch from the edge's 16-bit code in the
//     descriptor and the agents' bases, as this kernel did until r26.  (Measured and dropped, round 6: 64 consecutive 16-byte parts per load --
//     a quarter of the cache-line requests -- with the address handed from the edge's lane by ds_bpermute: the wave reached
//     the request hand-off 1.5 us LATER; and with the codes looked up per part: scalar loads inside every trip, 4 us later.)
//   * the streamers, coefficients: the packed copy [edge][16] (AgentDev::fe_coef) read straight through, 1 KB per wave and
//     load -- 100 cache-line requests where one lane per edge asked for 800 (the kernel's first microseconds are a count of
//     such requests: ~4400 per CU in front of the stream, and a CU's texture path takes about one a cycle).  Wave 7 did this
//     until r29, behind its other 35 requests and its count-in: see the head of the file.
template <int R>
struct FdXn {
  double2 v[3][2 * R];
};

// the front table's reads (step_front.h): ordinary vector loads, indexed by lane
__device__ __forceinline__ const double *fd_front_ld_xaddr(const FdFront *ft, int parity, int slot) {
  typedef const double *Ptr;
  return *(const __attribute__((address_space(1))) Ptr *)&ft->xaddr[parity][slot];
}

// (the record without its first word: the chain waves use {vs_off, pe0, pe1} only, and a word of a load that nobody reads is a
// register the compiler reuses while the load is in flight -- behind a wait for it, in the middle of the wave's requests)
struct FdFrontPubTail {
  int vs_off, pe0, pe1;
};

__device__ __forceinline__ FdFrontPubTail fd_front_ld_pub_tail(const FdFront *ft, int q) {
  static_assert(offsetof(FdFrontPub, vs_off) == 4 && offsetof(FdFrontPub, pe0) == 8 && offsetof(FdFrontPub, pe1) == 12, "12 bytes behind pose");
  typedef int v3i_t __attribute__((ext_vector_type(3), aligned(4)));
  const v3i_t v = *(const __attribute__((address_space(1))) v3i_t *)&ft->pub[q].vs_off;
  return FdFrontPubTail{v.x, v.y, v.z};
}

template <int R>
__device__ __forceinline__ void fd_xn_request(const double *const (&xa)[3], FdXn<R> &xr) {
  // (every slot, edges or not: loads under a wave-uniform `if` leave the compiler without a count of what is in flight behind
  // the join, and the wait in front of the LDS writes becomes a wait for EVERYTHING the wave has requested; the table's slots
  // beyond the last edge hold the address of a pose that exists)
#pragma unroll
  for (int q = 0; q < 3; ++q) {
#pragma unroll
    for (int k = 0; k < 2 * R; ++k) xr.v[q][k] = ld2(xa[q] + 2 * k);
  }
}

template <int R>
__device__ __forceinline__ void fd_xn_to_lds(int nshared, int ln, const FdXn<R> &xr, double *Es) {
  constexpr int EPE = 4 * R + 16;
  int nsh = nshared;
  // (held in a register: left as an expression of the descriptor the count was RE-READ from the kernel arguments in front of
  // every store below, each time behind a wait for the scalar load and the LDS store before it; read off the ISA, round 6)
  asm volatile("" : "+v"(nsh));
#pragma unroll
  for (int q = 0; q < 3; ++q) {
    if (64 * q < nsh && 64 * q + ln < nsh) {
      double *E = Es + (size_t)(64 * q + ln) * EPE;
#pragma unroll
      for (int k = 0; k < 2 * R; ++k) *reinterpret_cast<double2 *>(E + 2 * k) = xr.v[q][k];
    }
  }
}

// The streamers' 256 lanes cover the FE_MAX_EDGES * 8 parts of 16 bytes in five loads per lane (part 256 j + lane: a wave's
// 64 lanes one contiguous KB), every trip requested whatever the count (see fd_xn_request).  A lane beyond the last part
// takes the LAST part and, in fd_cf_to_lds, writes it to that part's own place -- the same value to the same address as the
// lane that owns it: the hand-off has no lane-varying branch and the compiler counts its waits (nshared >= 1 in every team
// that takes this form: fe_deep_m0).
struct FdCf {
  static constexpr int TRIPS = FE_MAX_EDGES * 8 / 256;
  static_assert(TRIPS * 256 == FE_MAX_EDGES * 8, "whole trips of the four streamer waves");
  double2 v[TRIPS];
  int t[TRIPS];  // the (clamped) part of each trip
};

__device__ __forceinline__ void fd_cf_request(const double *fe_coef, int nshared, int tid, FdCf &cr) {
  // (held in a register: left as an expression of the head the count is formed again in front of every store)
  // (never below part 0, whatever the head says: the allocation behind fe_coef and edge 0's place in LDS always exist)
  int last = max(nshared * 8 - 1, 0);
  asm volatile("" : "+v"(last));
#pragma unroll
  for (int j = 0; j < FdCf::TRIPS; ++j) {
    cr.t[j] = min(256 * j + tid, last);
    cr.v[j] = ld2(fe_coef + 2 * cr.t[j]);
  }
}

template <int R>
__device__ __forceinline__ void fd_cf_to_lds(const FdCf &cr, double *Es) {
  constexpr int EPE = 4 * R + 16;
#pragma unroll
  for (int j = 0; j < FdCf::TRIPS; ++j)
    *reinterpret_cast<double2 *>(Es + (cr.t[j] >> 3) * EPE + 4 * R + 2 * (cr.t[j] & 7)) = cr.v[j];
}

// the last NC chunks of one column per lane of waves 4-7 (lane l of the four: column group (l >> 5) & 7, k-lane l & 31 -- the
// mapping of k_step_fe's stream waves) and the partial sums the previous launch left for it: requested in front of barrier
// A; behind hand-off D the SAME chain of fused multiply-adds continues over the rows that are in LDS by then
template <int R, int NC>
struct FdCur {
  double2 mc[NC];
  double pa[R];
};

template <int R, int M0, int NC>
__device__ __forceinline__ void fd_cur_request(const FdHead &hd, int N4, int bx, int nblk, int l, FdCur<R, NC> &cu) {
  static_assert(NC <= FD_HEAD_ORD_MAX && M0 + NC == 32, "the head holds the ids of the last chunks");
  const int cg = (l >> 5) & 7, kl = l & 31;
  const int col = 8 * bx + cg;
  const double *pacc_in = hd.pacc_in;
  const double *Mc = hd.M + (size_t)((col < N4) ? col : 0) * N4;
#pragma unroll
  for (int i = 0; i < NC; ++i) cu.mc[i] = ld2_nt(Mc + min(2 * kl + 64 * fd_head_ord(hd.ord_lo, hd.ord_hi, i), N4 - 2));
#pragma unroll
  for (int a = 0; a < R; ++a) cu.pa[a] = gp(pacc_in)[((size_t)min(bx, nblk - 1) * R + a) * 256 + l];
}

template <int R, int M0, int NC>
__device__ __forceinline__ void fd_cur_product(const FdCur<R, NC> &cu, const double *vs, double *red, int l) {
  const int cg = (l >> 5) & 7, kl = l & 31;
  double acc[R];
#pragma unroll
  for (int a = 0; a < R; ++a) acc[a] = cu.pa[a];
#pragma unroll
  for (int i = 0; i < NC; ++i) {
    const int k = 2 * kl + 64 * (M0 + i);
    double wv[2 * R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const double2 t2 = *reinterpret_cast<const double2 *>(&vs[k * R + 2 * q]);
      wv[2 * q] = t2.x; wv[2 * q + 1] = t2.y;
    }
#pragma unroll
    for (int a = 0; a < R; ++a) acc[a] = __builtin_fma(wv[R + a], cu.mc[i].y, __builtin_fma(wv[a], cu.mc[i].x, acc[a]));
  }
#pragma unroll
  for (int a = 0; a < R; ++a) red[kl * (8 * R + 1) + cg * R + a] = acc[a];
}

#define FD_TRACE_PART (fd_args_behind_requests<false>().ag.part)
#ifdef DPGO_FE_TRACE
#ifndef DPGO_FE_TRACE_BLOCK
#define DPGO_FE_TRACE_BLOCK 100
#endif
#define FD_TRACE_DECL __shared__ unsigned long long fd_stamps[8 * 16];
#ifndef DPGO_FD_STAMP_MASK
#define DPGO_FD_STAMP_MASK 0xFFFF
#endif
#define FD_STAMP(k) do { if (((DPGO_FD_STAMP_MASK >> (k)) & 1) && (threadIdx.x & 63) == 0) fd_stamps[(threadIdx.x >> 6) * 16 + (k)] = wall_clock64(); } while (0)
#define FD_FLUSH() do { if ((threadIdx.x & 63) == 0) { const int w_ = threadIdx.x >> 6; \
    if (blockIdx.x == DPGO_FE_TRACE_BLOCK) for (int k_ = 0; k_ < 16; ++k_) FD_TRACE_PART[PART_E + 4000 * PART_STRIDE + w_ * 16 + k_] = (double)fd_stamps[w_ * 16 + k_]; \
    if (w_ == 4) { FD_TRACE_PART[PART_E + (4100 + 2 * (int)blockIdx.x) * PART_STRIDE] = (double)fd_stamps[4 * 16]; FD_TRACE_PART[PART_E + (4100 + 2 * (int)blockIdx.x) * PART_STRIDE + 1] = (double)fd_stamps[4 * 16 + 15]; } \
    if (w_ == 0) { FD_TRACE_PART[PART_E + (4100 + 2 * (int)blockIdx.x) * PART_STRIDE + 2] = (double)fd_stamps[15]; } } } while (0)
#elif defined(DPGO_FD_ENDS)
// -DDPGO_FD_ENDS: nothing but the time every wave of workgroup 100 leaves, straight to memory (one store per wave: the
// build runs within 0.1 us of the product build) -- PART_E words [4000 + 16 w + 15]; wave 4 also leaves its start [64]
#define FD_TRACE_DECL
#define FD_STAMP(k) do { if ((k) == 0 && blockIdx.x == 100 && threadIdx.x == 256) FD_TRACE_PART[PART_E + 4000 * PART_STRIDE + 64] = (double)wall_clock64(); } while (0)
#define FD_FLUSH() do { if (blockIdx.x == 100 && (threadIdx.x & 63) == 0) FD_TRACE_PART[PART_E + 4000 * PART_STRIDE + (threadIdx.x >> 6) * 16 + 15] = (double)wall_clock64(); } while (0)
#else
#define FD_TRACE_DECL
#define FD_STAMP(k) do { } while (0)
#define FD_FLUSH() do { } while (0)
#endif

// everything a launch is told beyond its head (step_head.h), by value in ONE struct behind it
struct FdArgs {
  AgentDev ag;
  FdNext nx;
  FeBases fb;
  TeamDev *team;
  const NestState *nest_src;
  NestState *nest_dst;
  double *pacc_out;
  double step;
  int sel, next_sel, next3_sel, num_robots, restart_interval, num_agents;
};

// The head arrives in registers; FdArgs (1.6 KB) sits in memory nobody has touched.  A role forms its first requests from
// the head alone and calls this BEHIND them: the struct as it may be read from here on -- the compiler can move no load of
// it above this point, where a wait for it would stand in front of those requests --, one word of each of its 64-byte lines
// touched first, all in flight at once (fetched where they are first used, every scalar load misses in turn; traced in round
// 6: the wave that needs the edges' codes issued its first request 2.7 us into the launch).  TOUCH = false: the streamers,
// which read it only behind the request hand-off.
// (The struct is addressed through the argument segment, where the launch ABI puts it: the arguments in order, each at its
// natural alignment.  Through the kernel's parameter the compiler would first copy all of it to scratch.)
constexpr size_t FD_ARGS_OFFSET = (4 * FD_HEAD_DWORDS + alignof(FdArgs) - 1) / alignof(FdArgs) * alignof(FdArgs);
template <bool TOUCH>
__device__ __forceinline__ const FdArgs &fd_args_behind_requests() {
  typedef const __attribute__((address_space(4))) char *SegPtr;
  __builtin_amdgcn_sched_barrier(0);
  SegPtr p = (SegPtr)__builtin_amdgcn_kernarg_segment_ptr() + FD_ARGS_OFFSET;
  asm volatile("" : "+s"(p)::"memory");
#if DPGO_FD_KA_PREFETCH
  if constexpr (TOUCH) {
    // (every 64th byte and the last word -- the struct does not start on a line --, consumed TOGETHER: folded into one word
    // the compiler fetched them in groups of eight, a wait and a cold trip for each group)
    const __attribute__((address_space(4))) unsigned *ka = (const __attribute__((address_space(4))) unsigned *)p;
    static_assert(sizeof(FdArgs) > 19 * 64 && sizeof(FdArgs) <= 20 * 64, "one operand below for every line of FdArgs");
    constexpr int LAST = (int)(sizeof(FdArgs) / 4) - 1;
    asm volatile("" ::"s"(ka[0]), "s"(ka[16]), "s"(ka[32]), "s"(ka[48]), "s"(ka[64]), "s"(ka[80]), "s"(ka[96]), "s"(ka[112]),
                 "s"(ka[128]), "s"(ka[144]), "s"(ka[160]), "s"(ka[176]), "s"(ka[192]), "s"(ka[208]), "s"(ka[224]), "s"(ka[240]),
                 "s"(ka[256]), "s"(ka[272]), "s"(ka[288]), "s"(ka[304]), "s"(ka[LAST]));
  }
#endif
  return *(const FdArgs *)p;
}

template <int R, int M0>
__global__ __launch_bounds__(512) void k_step_fd(double *hd_buf0, const double *hd_M, const double *__restrict__ hd_pacc_in,
                                                 const double *hd_fe_coef, unsigned hd_np, unsigned hd_sf, unsigned hd_ord_lo,
                                                 unsigned hd_ord_hi, int nblk_all, const FdArgs fa) {
  // ---- the head (step_head.h): nothing down to the roles' calls of fd_args_behind_requests reads anything else
  const FdHead hd = {hd_buf0, hd_M, hd_pacc_in, hd_fe_coef, hd_np, hd_sf, hd_ord_lo, hd_ord_hi, nblk_all};
  const int n = fd_head_n(hd.np), N4 = 4 * n, hd_npub = fd_head_npub(hd.np), hd_nshared = fd_head_nshared(hd.sf);
  const int parity = fd_head_parity(hd.sf), flags = fd_head_flags(hd.sf);
  const FdFront *ft = fd_front_of(hd.fe_coef);  // the front table (step_front.h): behind the coefficients, at a fixed offset
  // the poses live twice (step_fused.hip): this launch reads the copy of its parity and writes the other one
  const double *__restrict__ Xr = fd_head_buf(hd.buf0, R, n, parity ? B_XALT : B_X);
  const double *__restrict__ Yr = fd_head_buf(hd.buf0, R, n, parity ? B_YALT : B_Y);
  double *__restrict__ Xw = fd_head_buf(hd.buf0, R, n, parity ? B_X : B_XALT);
  double *__restrict__ Yw = fd_head_buf(hd.buf0, R, n, parity ? B_Y : B_YALT);
  const int hb = (int)blockIdx.x;
  // XCD-aware block order, as in k_precond.  (The grid is nblk_all rounded up to a multiple of 8, launch_step_fd: gridDim
  // itself is a word of the hidden arguments, behind FdArgs)
  const int bx = (hb % 8) * ((nblk_all + 7) / 8) + hb / 8;
  const int tid = threadIdx.x;
  const int nblk = (N4 + 7) / 8;
  if (bx >= nblk_all) return;
  // (the grid covers the largest agent of the team: a workgroup beyond this agent's columns still takes its share of the
  // other agents' work)
  const bool own = bx < nblk, in = (flags & FD_IN) != 0;
  constexpr int KC = FD_KC, MREG = KC / 64, NC = MREG - M0;
  __shared__ double vs[R * KC];  // chunk-ordered: [0, M0 * 64 R) the private rows of the NEXT agent's carried gradient, behind
                                 // them the rows of THIS agent's gradient that the last NC chunks meet
  __shared__ double zs[8 * R];
  __shared__ double red[32 * (8 * R + 1)];
  __shared__ double Ysh[2 * 4 * R];
  __shared__ double Esh[2][2 * 4 * R];
  __shared__ double Es[FE_MAX_EDGES * (4 * R + 16)];
  __shared__ double tl_x[2 * 4 * R], tl_v[2 * 4 * R], tl_y[2 * 4 * R], tl_s[2 * 16];
  __shared__ double Ex[2 * 3 * 4 * R];
  __shared__ double Psh[2 * 4 * R], tl_rel[2];  // XPrev of the two poses, their |X - XPrev|^2 (steps that leave statistics)
  __shared__ int sy[FD_SY_COUNT];
  FD_TRACE_DECL
  FD_STAMP(0);
  if (tid < FD_SY_COUNT) sy[tid] = 0;
  lds_barrier();  // Z: the counters are zero (the only workgroup barrier; every wave is here within its first instructions)
  const int pj0 = own ? 2 * bx : 0, pj1 = (own && 2 * bx + 1 < n) ? 2 * bx + 1 : -1;
  const int npose = own ? ((pj1 >= 0) ? 2 : 1) : 0;
  constexpr int EPE = 4 * R + 16;
  const int cwv = __builtin_amdgcn_readfirstlane(tid >> 6), ln = tid & 63;

  if (cwv < 4) {
    // ================================================================ streamers
    const int cg = (tid >> 5) & 7, kl = tid & 31;
    // the coefficients of the shared edges, FIRST: the chain waits for them (E) and for nothing else it does not hold by then
    fd_role_entry<FD_ROLE_STREAM>();
    FdCf cf;
    fd_cf_request(hd.fe_coef, hd_nshared, tid, cf);
    // the rows of this agent's carried gradient that the last NC chunks meet: positions [M0 * 64 R, N4 R)
    constexpr int NGC = ((KC - 64 * M0) * R / 2 + 255) / 256;
    double2 gc[NGC];
    const double *Gc = fd_head_buf(hd.buf0, R, n, B_CARRY_G);
#if !DPGO_FD_GC_LATE
    {
#pragma unroll
      for (int u = 0; u < NGC; ++u) gc[u] = ld2(Gc + min(M0 * 64 * R + 2 * (tid + 256 * u), N4 * R - 2));
    }
#endif
    // (vmcnt retires in order: the writes below wait for the coefficients alone and leave the carried rows in flight)
    __builtin_amdgcn_sched_barrier(0);
    fd_cf_to_lds<R>(cf, Es);
    fd_signal_coef(&sy[FD_SY_E]);
    FD_STAMP(8);
    for (int t = N4 * R + tid; t < KC * R; t += 256) vs[t] = 0.0;  // rows beyond the agent's
    // (FdArgs behind the hand-off E: its scalar loads share the counter the hand-off's fence waits for.  The streamers touch
    // none of its lines up front -- waves 4-7 do --: the chain needs the carried rows only behind its gradient phase, and the
    // stream waits for the request hand-off anyway)
    const FdArgs &as = fd_args_behind_requests<false>();
    const FdNext &nx = as.nx;
    const int cold = 8 * bx + cg;
    const int N4d = nx.N4d;
    const double *Md = nx.Md + (size_t)((cold < N4d) ? cold : 0) * N4d;
    double2 mn[M0];
    FD_STAMP(10);
    __builtin_amdgcn_sched_barrier(0);
#if DPGO_FD_GC_LATE
    {
#pragma unroll
      for (int u = 0; u < NGC; ++u) gc[u] = ld2(Gc + min(M0 * 64 * R + 2 * (tid + 256 * u), N4 * R - 2));
    }
#endif
#pragma unroll
    for (int u = 0; u < NGC; ++u) {
      const int tt = M0 * 64 * R + 2 * (tid + 256 * u);
      if (tt < N4 * R) *reinterpret_cast<double2 *>(&vs[tt]) = gc[u];
    }
    fd_signal(&sy[FD_SY_C]);
    FD_STAMP(1);
    fd_wait(&sy[FD_SY_RQ], 4);  // A: waves 4-7 have requested all they need -- the stream queues behind it, not in front
    FD_STAMP(11);
    // (nothing of the stream is requested in front of this hand-off: a wave stays at the issue of such loads, and the chain
    // waits for C -- the scheduler otherwise hoists the requests above the LDS writes)
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("" ::: "memory");
    // ---- P: the private chunks of the next agent's M against the private rows of its carried gradient
    constexpr int NGN = (M0 * 64 * R / 2 + 255) / 256;
    double2 gn[NGN];
#pragma unroll
    for (int u = 0; u < NGN; ++u) gn[u] = ld2(nx.Gd + min(2 * (tid + 256 * u), M0 * 64 * R - 2));
    // (every row of the vector requested in front of the first load of M, and written without a guard -- a lane beyond the
    // last pair writes the clamped pair to its own place: a row load the scheduler moves in among the loads of M, or sinks
    // into a guarded write, puts a wait for the WHOLE stream in front of the hand-off N, and the product then starts behind
    // the last chunk's data where it can follow the chunks as they land: its waits are counted, vmcnt(M0 - 1) ... (0))
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("; fd_stream_entry 0");
#pragma unroll
    for (int i = 0; i < M0; ++i) mn[i] = ld2_nt(Md + min(2 * kl + 64 * (int)nx.ord_d[i], N4d - 2));
    FD_STAMP(12);
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int u = 0; u < NGN; ++u) *reinterpret_cast<double2 *>(&vs[min(2 * (tid + 256 * u), M0 * 64 * R - 2)]) = gn[u];
    asm volatile("; fd_n_count 0" ::: "memory");
    fd_signal(&sy[FD_SY_N]);
    fd_wait(&sy[FD_SY_N], 4);
    fd_wait(&sy[FD_SY_F], 4);  // (the chain's product first: the two share the LDS)
    FD_STAMP(13);
    double acc[R];
#pragma unroll
    for (int a = 0; a < R; ++a) acc[a] = 0;
#pragma unroll
    for (int i = 0; i < M0; ++i) {
      if (i % 8 == 0 && i > 0) {
        // (the rows of no more than eight chunks read ahead of their multiply-adds: beside the slab's 96 registers the 36
        // reads the scheduler otherwise hoists above the first multiply-add fit only by luck, and a spill is scratch
        // traffic in the queue the chain waits on)
#pragma unroll
        for (int a = 0; a < R; ++a) asm volatile("" : "+v"(acc[a])::"memory");
      }
      const int k = 2 * kl + 64 * i;
      double wv[2 * R];
#pragma unroll
      for (int q = 0; q < R; ++q) {
        const double2 t2 = *reinterpret_cast<const double2 *>(&vs[k * R + 2 * q]);
        wv[2 * q] = t2.x; wv[2 * q + 1] = t2.y;
      }
#pragma unroll
      for (int a = 0; a < R; ++a) acc[a] = __builtin_fma(wv[R + a], mn[i].y, __builtin_fma(wv[a], mn[i].x, acc[a]));
    }
    if ((flags & FD_P) && bx < nx.nblk_d) {
#pragma unroll
#if DPGO_FD_PACC_WT
      for (int a = 0; a < R; ++a) st_c(as.pacc_out + ((size_t)bx * R + a) * 256 + tid, acc[a]);  // (write-through: not left dirty in L2 for the kernel boundary)
#else
      for (int a = 0; a < R; ++a) gp(as.pacc_out)[((size_t)bx * R + a) * 256 + tid] = acc[a];
#endif
    }
    FD_STAMP(15);
    FD_FLUSH();
    return;
  }

  if (cwv < 6) {
    // ================================================================ the chain: gradient of the public poses, product over the
    // last chunks, step of the workgroup's poses
    const int g = cwv - 4;
    fd_role_entry<FD_ROLE_CHAIN>();
    // ---- from the head: W / X of the public poses, this wave's quarter of the last chunks, the operands of the tail
    const int npub = hd_npub;
    const int pq = 64 * g + ln;
    const bool pact = pq < npub;
    const int pqc = pact ? pq : 0;
    // (the lane's public pose -- where its row goes, which edges are its -- from the front table, first: one 12-byte load;
    // records beyond the last public pose are zeros)
    const FdFrontPubTail pr = fd_front_ld_pub_tail(ft, pq);
    __builtin_amdgcn_sched_barrier(0);
    // (of the point only the rotation block is read, tangent_inplace: its 3r entries are requested, nothing of the translation
    // column -- a pair that straddles the two as 8 bytes, see fd_front_ld_pub_tail)
    double w[4 * R], x[3 * R];
    {
      const double *Wc = fd_head_buf(hd.buf0, R, n, B_CARRY_W), *Xc = fd_head_buf(hd.buf0, R, n, B_CARRY_X);
#pragma unroll
      for (int i = 0; i < 2 * R; ++i) {
        // ([entry pair][public pose][2]: one 16-byte load per pair, a wave's 64 lanes one contiguous KB -- half the requests)
        const double2 tw = ld2(Wc + ((size_t)i * npub + pqc) * 2);
        w[2 * i] = tw.x; w[2 * i + 1] = tw.y;
        if (2 * i + 1 < 3 * R) {
          const double2 tx = ld2(Xc + ((size_t)i * npub + pqc) * 2);
          x[2 * i] = tx.x; x[2 * i + 1] = tx.y;
        } else if (2 * i < 3 * R) {
          x[2 * i] = gp(Xc)[((size_t)i * npub + pqc) * 2];
        }
      }
    }
    FD_STAMP(14);
    FdCur<R, NC> cu;
    fd_cur_request<R, M0, NC>(hd, N4, bx, nblk, tid - 256, cu);
    // operands of the tail (the lanes of wave 4 that will hold them; wave 5's copies are never used)
    const int tl = tid - 256 - 64 * g;
    const size_t own_off = (size_t)((tl >= 4 * R) ? max(pj1, 0) : pj0) * 4 * R + (size_t)(tl % (4 * R));
    double pre_x = 0, pre_v = 0, pre_y = 0, pre_p = 0;
    if (tl < npose * 4 * R) {
      pre_x = gp(Xr)[own_off];
      pre_v = gp(fd_head_buf(hd.buf0, R, n, B_V))[own_off];
      pre_y = gp(Yr)[own_off];
      pre_p = gp(fd_head_buf(hd.buf0, R, n, B_XPREV))[own_off];
    }
    // ---- behind them, from FdArgs: the rows of W, the Nesterov state
    const FdArgs &as = fd_args_behind_requests<true>();
    const AgentDev &ag = as.ag;
    const FdNext &nx = as.nx;
    const int pe0 = pr.pe0, pe1 = pr.pe1, vs_off = pr.vs_off;
    // W (wave 5, behind its quarter of the product): the indices of the rows now (wave 4's copies are never used)
    const int npw = (nx.n_e + nblk_all - 1) / nblk_all;  // (<= 2)
    const int wls = ln / (4 * R), we = ln - wls * (4 * R);
    const int pw = bx * npw + wls;
    const bool pv = wls < 3 && wls < npw && pw < nx.n_e;
    const int pwc = pv ? pw : 0;
    const int wtile = pwc >> 6, wpl = pwc & 63, wdn = nx.soa_w_e;
    int ii[8];
#pragma unroll
    for (int u = 0; u < 8; ++u) ii[u] = gp(nx.soa_col_e)[((size_t)wtile * wdn + min(u, wdn - 1)) * 64 + wpl];
    const int qi = gp(nx.pub_index_e)[pwc];
    const int sel = as.sel, next_sel = as.next_sel, num_robots = as.num_robots, restart_interval = as.restart_interval;
    const FdNestReq nrq = fd_nest_request(as.nest_src + sel);
    __builtin_amdgcn_s_setprio(3);  // (the chain's instructions go first: the streamers' product shares the LDS with it)
    FD_STAMP(10);
    fd_signal_requested<FD_ROLE_CHAIN>(&sy[FD_SY_RQ]);
    FD_STAMP(11);
    fd_wait(&sy[FD_SY_E], 5);  // the operands of the shared edges are in LDS: wave 6's poses, the four streamers' coefficients
    FD_STAMP(1);
    if (pact) {
      // G_j from LDS: g[c][a] -= x[cp][a] coef[cp + 4c], edge after edge and cp after cp for every entry (g_row_range's order)
      double gg[4 * R];
#pragma unroll
      for (int i = 0; i < 4 * R; ++i) gg[i] = 0.0;
      for (int e = pe0; e < pe1; ++e) {
        const double *E = Es + (size_t)e * EPE;
        double xn[4 * R];
#pragma unroll
        for (int i = 0; i < 2 * R; ++i) { const double2 t = *reinterpret_cast<const double2 *>(E + 2 * i); xn[2 * i] = t.x; xn[2 * i + 1] = t.y; }
#pragma unroll
        for (int c = 0; c < 4; ++c) {
          const double2 c01 = *reinterpret_cast<const double2 *>(E + 4 * R + 4 * c), c23 = *reinterpret_cast<const double2 *>(E + 4 * R + 4 * c + 2);
          const double cfc[4] = {c01.x, c01.y, c23.x, c23.y};
#pragma unroll
          for (int cp = 0; cp < 4; ++cp)
#pragma unroll
            for (int a = 0; a < R; ++a) gg[c * R + a] -= xn[cp * R + a] * cfc[cp];
        }
      }
#pragma unroll
      for (int i = 0; i < 4 * R; ++i) w[i] = w[i] + gg[i];
      tangent_inplace<R>(x, w);
    }
    FD_STAMP(3);
    fd_wait(&sy[FD_SY_C], 4);  // the carried rows are in LDS: the public ones are overwritten now
    FD_STAMP(2);
    if (pact) {
#pragma unroll
      for (int i = 0; i < 4 * R; ++i) vs[vs_off + i] = w[i];
    }
    FD_STAMP(12);
    fd_signal(&sy[FD_SY_D]);
    FD_STAMP(13);
    fd_wait(&sy[FD_SY_D], 2);
    FD_STAMP(4);
    fd_cur_product<R, M0, NC>(cu, vs, red, tid - 256);
    if (tl >= 0 && tl < npose * 4 * R) { Ysh[tl] = pre_x; Esh[0][tl] = pre_v; Esh[1][tl] = pre_y; Psh[tl] = pre_p; }
    FD_STAMP(5);
    fd_signal(&sy[FD_SY_F]);
    if (g == 1) {
      // ---- W: the row products of agent e at the point B_CARRY_Y holds (left complete by the previous launch), for this
      // workgroup's share of its poses -- one (pose, entry) per lane, fe_block's expression slot after slot (bitwise the sums
      // a self-forming launch would make), then their tangent projection at the point
      __builtin_amdgcn_s_setprio(0);
      const int c = we / R, a = we - c * R;
      const double *__restrict__ Y2 = nx.Ye;
      double xv[8][4], bv[8][4];
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double *xp = Y2 + (size_t)4 * R * ii[u] + a;
        const double *bp = nx.soa_val_e + ((size_t)wtile * wdn + min(u, wdn - 1)) * 1024 + (2 * c) * 128 + 2 * wpl;
        xv[u][0] = gp(xp)[0]; xv[u][1] = gp(xp)[R]; xv[u][2] = gp(xp)[2 * R]; xv[u][3] = gp(xp)[3 * R];
        bv[u][0] = gp(bp)[0]; bv[u][1] = gp(bp)[1]; bv[u][2] = gp(bp)[128]; bv[u][3] = gp(bp)[129];
      }
      const double xe_ = gp(Y2)[(size_t)4 * R * pwc + we];
      double acc = 0.0;
#pragma unroll
      for (int u = 0; u < 8; ++u) {
        const double t = fma4(xv[u][0], bv[u][0], xv[u][1], bv[u][1], xv[u][2], bv[u][2], xv[u][3], bv[u][3], acc);
        acc = (u < wdn) ? t : acc;
      }
      const bool wr = pv && (flags & FD_W);
      if (wr && qi >= 0) {  // (a public pose: its launch finishes it -- row product and point, [entry][public pose])
        gp(nx.We)[((size_t)(we >> 1) * nx.npub_e + qi) * 2 + (we & 1)] = acc;
        gp(nx.Xe)[((size_t)(we >> 1) * nx.npub_e + qi) * 2 + (we & 1)] = xe_;
      }
      if (wls < 3) { Ex[wls * 4 * R + we] = acc; Ex[3 * 4 * R + wls * 4 * R + we] = xe_; }
      WSYNC();
      if (wr && we == 0) {
        double ww[4 * R], xx[4 * R];
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) { ww[i] = Ex[wls * 4 * R + i]; xx[i] = Ex[3 * 4 * R + wls * 4 * R + i]; }
        tangent_inplace<R>(xx, ww);
        double *Gn = nx.Ge + fd_pos_off<R>(nx.ord_e, pw);  // (chunk-ordered: the launches that consume it copy straight ranges)
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) gp(Gn)[i] = ww[i];
      }
      FD_STAMP(14);
      FD_FLUSH();
      return;
    }
    fd_wait(&sy[FD_SY_F], 4);
    if (ln < 8 * R) {
      double s = 0;
#pragma unroll
      for (int q = 0; q < 32; ++q) s += red[q * (8 * R + 1) + ln];
      zs[ln] = s;
    }
    FD_STAMP(6);
    WSYNC();
    // (the state is brought to scalar registers HERE, where it is first used: the wait for it is a wait for everything the wave
    // has requested, and directly behind the count-in it stood in front of the chain's first phase)
    const NestState ns = fd_nest_state(nrq);
    const NestAhead nn = nest_ahead(ns, num_robots, restart_interval);
    const bool ahead_opt = next_sel == sel;
    const bool stats = in && (flags & FD_STATS) != 0, lastat = in && (flags & FD_LASTAT) != 0;
    if (ln < 2) tl_rel[ln] = 0.0;
    // ---- the step of the workgroup's two poses, one pose on 16 lanes
    const TwoPoseLds tl2 = {zs, Ysh, Esh[0], Esh[1], Psh, tl_x, tl_v, tl_y, tl_s, tl_rel};
    step_two_poses<R>(ag, Xw, Yw, tl2, ln, npose, pj0, pj1, as.step, nn, ahead_opt, in, stats, lastat, [&](int k) { FD_STAMP(k); });
    if (stats) {
      // (k_precond: the two poses' sums through wave_sum, lane 0 stores)
      WSYNC();
      double rl = (ln < npose) ? tl_rel[ln] : 0.0;
      rl = wave_sum(rl);
      if (ln == 0 && own) gp(ag.part)[PART_B + (size_t)bx * PART_STRIDE + 2] = rl;
    }
    FD_STAMP(15);
    FD_FLUSH();
    return;
  }

  // ================================================================ waves 6 and 7: the operands of the shared edges into LDS,
  // then the row products of the agent two iterations ahead (6) / the look-ahead of the other agents' poses (7)
  const int h = cwv - 6;
  if (h == 0) {
    // (where its three edges' neighbour poses live, from the front table, FIRST: its quarter of the last chunks is requested
    // while the addresses travel, and the wait in front of the pose loads counts the three address loads alone)
    fd_role_entry<FD_ROLE_POSES>();
    const double *xa[3];
#pragma unroll
    for (int q = 0; q < 3; ++q) xa[q] = fd_front_ld_xaddr(ft, parity, 64 * q + ln);
    __builtin_amdgcn_sched_barrier(0);
    FdCur<R, NC> cu;
    fd_cur_request<R, M0, NC>(hd, N4, bx, nblk, tid - 256, cu);
    FdXn<R> er;
    fd_xn_request<R>(xa, er);
    FD_STAMP(9);
    const FdArgs &as = fd_args_behind_requests<true>();
    FD_STAMP(10);
    fd_signal_requested<FD_ROLE_POSES>(&sy[FD_SY_RQ]);
    FD_STAMP(11);
    __builtin_amdgcn_s_setprio(3);
    fd_xn_to_lds<R>(hd_nshared, ln, er, Es);
    fd_signal(&sy[FD_SY_E]);
    FD_STAMP(8);
    fd_wait(&sy[FD_SY_D], 2);  // this wave's quarter of the product over the last chunks
    fd_cur_product<R, M0, NC>(cu, vs, red, tid - 256);
    fd_signal(&sy[FD_SY_F]);
    if (bx == 0 && ln < LOOKAHEAD_MAX_AGENTS && in)  // the books, one lane per agent
      step_books(as.team, as.nest_src, as.nest_dst, ln, as.num_agents, as.sel, as.next_sel, as.num_robots, as.restart_interval);
    FD_STAMP(14);
    FD_FLUSH();
    return;
  }

  // ---- wave 7: look-ahead Nesterov step of iteration k+1 for this workgroup's share of the OTHER agents' poses (one lane
  // per pose, k_step_fe's second wave), every address from the launch's arguments
  {
    fd_role_entry<FD_ROLE_COEF>();
    FdCur<R, NC> cu;
    fd_cur_request<R, M0, NC>(hd, N4, bx, nblk, tid - 256, cu);
    FD_STAMP(9);
    const FdArgs &as = fd_args_behind_requests<true>();
    const FeBases &fb = as.fb;
    const int sel = as.sel, next_sel = as.next_sel, next3_sel = as.next3_sel, num_agents = as.num_agents;
    const int num_robots = as.num_robots, restart_interval = as.restart_interval;
    int pre[LOOKAHEAD_MAX_AGENTS + 1];
    pre[0] = 0;
#pragma unroll
    for (int k = 0; k < LOOKAHEAD_MAX_AGENTS; ++k) pre[k + 1] = pre[k] + ((k < num_agents) ? fb.npose[k] : 0);
    const int total = pre[LOOKAHEAD_MAX_AGENTS] - n;
    const int per = (total + nblk_all - 1) / nblk_all;  // <= 64, checked by the host
    const int q = bx * per + ln;
    const bool lact = ln < per && q < total;
    int self_lo = 0;
#pragma unroll
    for (int k = 0; k < LOOKAHEAD_MAX_AGENTS; ++k) if (k == sel) self_lo = pre[k];
    const int gq = lact ? (q < self_lo ? q : q + n) : 0;
    // (the lane's agent: its Y array and pose count are VALUES selected among the eight the wave holds in scalar registers.
    // Left as a choice among fb's fields the compiler selects the field's ADDRESS per lane and fetches the two with vector
    // loads from the argument segment -- a dependent trip, queued behind the coefficients and M, in front of the wave's first
    // look-ahead address.  The address is an integer while it is chosen and a global pointer again behind it: the accesses
    // below stay global_ ones -- one flat access in the kernel and the compiler's counted waits become waits for everything)
    unsigned long long yb[LOOKAHEAD_MAX_AGENTS];
    int nb[LOOKAHEAD_MAX_AGENTS];
#pragma unroll
    for (int k = 0; k < LOOKAHEAD_MAX_AGENTS; ++k) {
      yb[k] = (unsigned long long)fb.ybase[k]; nb[k] = fb.npose[k];
      asm volatile("" : "+s"(yb[k]), "+s"(nb[k]));
    }
    int a = 0, lo = 0, na_ = nb[0];
    unsigned long long yau = yb[0];
#pragma unroll
    for (int k = 1; k < LOOKAHEAD_MAX_AGENTS; ++k)
      if (k < num_agents && gq >= pre[k]) { a = k; lo = pre[k]; yau = yb[k]; na_ = nb[k]; }
    // (the work vectors of an agent are one allocation, NBUF x (4r n): everything from its Y array)
    const size_t vlen = (size_t)4 * R * na_;
    double *yp = (double *)(__attribute__((address_space(1))) double *)yau;
    double *xa = yp - (size_t)(B_Y - B_X) * vlen, *va = yp + (size_t)(B_V - B_Y) * vlen;
    const size_t da = (size_t)B_ALT * vlen;
    const double *xr = parity ? xa + da : xa, *yr = parity ? yp + da : yp;
    double *oX = parity ? xa : xa + da, *oY = parity ? yp : yp + da, *oV = va;
    const int la_pose = gq - lo;
    const bool la_opt = next_sel == a;
    const size_t o = (size_t)la_pose * 4 * R;
    double la_x[4 * R], la_v[4 * R];
#pragma unroll
    for (int i = 0; i < 2 * R; ++i) {
      const double2 tx = ld2(xr + o + 2 * i), tv = ld2(va + o + 2 * i);
      la_x[2 * i] = tx.x; la_x[2 * i + 1] = tx.y; la_v[2 * i] = tv.x; la_v[2 * i + 1] = tv.y;
    }
    const FdNestReq nrq = fd_nest_request(as.nest_src + sel);
    FD_STAMP(10);
    fd_signal_requested<FD_ROLE_COEF>(&sy[FD_SY_RQ]);
    FD_STAMP(11);
    __builtin_amdgcn_s_setprio(3);
    fd_wait(&sy[FD_SY_D], 2);  // this wave's quarter of the product over the last chunks
    fd_cur_product<R, M0, NC>(cu, vs, red, tid - 256);
    fd_signal(&sy[FD_SY_F]);
    __builtin_amdgcn_s_setprio(0);
    // (the state: consumed here, behind the product -- directly behind the count-in the wait for it, which is a wait for all the
    // wave has requested, stood in front of the coefficients' hand-off E)
    const NestState ns = fd_nest_state(nrq);
    const NestAhead nn = nest_ahead(ns, num_robots, restart_interval);
    if (lact) {
      const bool st = in, lastat = in && (flags & FD_LASTAT) != 0;
      double *pa_ = fb.part[0];
#pragma unroll
      for (int k = 1; k < LOOKAHEAD_MAX_AGENTS; ++k) pa_ = (a == k) ? fb.part[k] : pa_;
      if (lastat) {
        double *xprev = yp - (size_t)(B_Y - B_XPREV) * vlen;
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) gp(xprev)[o + i] = la_x[i];
      }
      if (nn.restart_next) {
        // (X stays; Y = V = X unless the agent optimizes next -- then Y stays too: both are carried into the other copy)
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) {
          if (st) oX[o + i] = la_x[i];
          if (!la_opt) { if (st) { oY[o + i] = la_x[i]; oV[o + i] = la_x[i]; } la_v[i] = la_x[i]; }
          else if (st) oY[o + i] = yr[o + i];
        }
        if (lastat && !la_opt) gp(pa_)[PART_D + la_pose] = 0.0;
      } else {
        double y[4 * R];
        lookahead_map<R>(la_x, la_v, nn.ahead_alpha, y);
        if (lastat && !la_opt) {
          double r2 = 0;
#pragma unroll
          for (int i = 0; i < 4 * R; ++i) { const double d = y[i] - la_x[i]; r2 += d * d; }
          gp(pa_)[PART_D + la_pose] = r2;
        }
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) { if (st) { oY[o + i] = y[i]; oX[o + i] = y[i]; } la_x[i] = y[i]; }
      }
      FD_STAMP(7);
      if ((flags & FD_Y) && a == next3_sel) {
        // Y: the point the agent of iteration k+3 will be evaluated at -- what the look-ahead waves of the next two launches
        // will leave in its X array (the same expressions on the same operands: bitwise), formed two launches early.  The
        // agent rests in k+1 and k+2; la_x / la_v hold its X and V after iteration k+1 here.
        if (nn.restart_next2) {
#pragma unroll
          for (int i = 0; i < 4 * R; ++i) la_v[i] = la_x[i];  // (k+2 restarts: X stays, V = Y = X)
        } else {
          double y[4 * R];
          lookahead_map<R>(la_x, la_v, nn.ahead2_alpha, y);
#pragma unroll
          for (int i = 0; i < 4 * R; ++i) la_x[i] = y[i];
        }
        if (!nn.restart_next3) {
          double y[4 * R];
          lookahead_map<R>(la_x, la_v, nn.ahead3_alpha, y);
#pragma unroll
          for (int i = 0; i < 4 * R; ++i) la_x[i] = y[i];
        }
        double *py3 = yp + (size_t)(B_CARRY_Y - B_Y) * (long long)vlen;
#pragma unroll
        for (int i = 0; i < 4 * R; ++i) gp(py3)[o + i] = la_x[i];
      }
    }
    FD_STAMP(15);
    FD_FLUSH();
  }
}

// the evaluation points of the first three agents of a run, from the state k_nest_pre leaves (every agent at its point of
// iteration 0): role 0 -- sel(0): the point itself; role 1 -- sel(1): one look-ahead map; role 2 -- sel(2): two.  The
// expressions are the look-ahead waves' (bitwise what launches 0 and 1 will leave in those agents' X arrays).
template <int R>
__global__ __launch_bounds__(64) void k_fd_prime(const AgentDev *__restrict__ agents, int s0, int s1, int s2, int num_robots,
                                                 int restart_interval, const NestState *nest_src) {
  const int role = (int)blockIdx.y;
  const int ai = role == 0 ? s0 : (role == 1 ? s1 : s2);
  const AgentDev &ag = agents[ai];
  const int j = (int)blockIdx.x * 64 + (int)threadIdx.x;
  if (j >= ag.n) return;
  const size_t o = (size_t)j * 4 * R;
  double x[4 * R], v[4 * R];
#pragma unroll
  for (int i = 0; i < 4 * R; ++i) { x[i] = gp(ag.buf[B_X])[o + i]; v[i] = gp(ag.buf[B_V])[o + i]; }
  const NestAhead nn = nest_ahead(nest_src[s0], num_robots, restart_interval);
  if (role == 2) {
    if (nn.restart_next) {
#pragma unroll
      for (int i = 0; i < 4 * R; ++i) v[i] = x[i];
    } else {
      double y[4 * R];
      lookahead_map<R>(x, v, nn.ahead_alpha, y);
#pragma unroll
      for (int i = 0; i < 4 * R; ++i) x[i] = y[i];
    }
  }
  if (role >= 1) {
    const bool rs = role == 1 ? nn.restart_next : nn.restart_next2;
    const double al = role == 1 ? nn.ahead_alpha : nn.ahead2_alpha;
    if (!rs) {
      double y[4 * R];
      lookahead_map<R>(x, v, al, y);
#pragma unroll
      for (int i = 0; i < 4 * R; ++i) x[i] = y[i];
    }
  }
#pragma unroll
  for (int i = 0; i < 4 * R; ++i) gp(ag.buf[B_CARRY_Y])[o + i] = x[i];
}

// The two producers a run opens with, as launches of their own (they used to be two full k_step_fd launches whose iteration
// part computed on nothing and stored nothing: 12 us each where these take a few).
// k_fd_rows: W for the agents sel(0) and sel(1) (blockIdx.y) from the points k_fd_prime left -- the W wave of k_step_fd,
// expression for expression, one wave per workgroup's share of the agent's poses.
template <int R>
__global__ __launch_bounds__(64) void k_fd_rows(const AgentDev *__restrict__ agents, int e0, int e1, int nblk_all) {
  const AgentDev &age = agents[blockIdx.y == 0 ? e0 : e1];
  const int bx = (int)blockIdx.x, ln = (int)threadIdx.x;
  __shared__ double Ex[2 * 3 * 4 * R];
  const int npw = (age.n + nblk_all - 1) / nblk_all;  // (<= 2)
  const int wls = ln / (4 * R), we = ln - wls * (4 * R);
  const int pw = bx * npw + wls;
  const bool pv = wls < 3 && wls < npw && pw < age.n;
  const int pwc = pv ? pw : 0;
  const int wtile = pwc >> 6, wpl = pwc & 63, wdn = age.soa_w;
  int ii[8];
#pragma unroll
  for (int u = 0; u < 8; ++u) ii[u] = gp(age.soa_col)[((size_t)wtile * wdn + min(u, wdn - 1)) * 64 + wpl];
  const int qi = gp(age.pub_index)[pwc];
  const int c = we / R, a = we - c * R;
  const double *__restrict__ Y2 = age.buf[B_CARRY_Y];
  double xv[8][4], bv[8][4];
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const double *xp = Y2 + (size_t)4 * R * ii[u] + a;
    const double *bp = age.soa_val + ((size_t)wtile * wdn + min(u, wdn - 1)) * 1024 + (2 * c) * 128 + 2 * wpl;
    xv[u][0] = gp(xp)[0]; xv[u][1] = gp(xp)[R]; xv[u][2] = gp(xp)[2 * R]; xv[u][3] = gp(xp)[3 * R];
    bv[u][0] = gp(bp)[0]; bv[u][1] = gp(bp)[1]; bv[u][2] = gp(bp)[128]; bv[u][3] = gp(bp)[129];
  }
  const double xe_ = gp(Y2)[(size_t)4 * R * pwc + we];
  double acc = 0.0;
#pragma unroll
  for (int u = 0; u < 8; ++u) {
    const double t = fma4(xv[u][0], bv[u][0], xv[u][1], bv[u][1], xv[u][2], bv[u][2], xv[u][3], bv[u][3], acc);
    acc = (u < wdn) ? t : acc;
  }
  if (pv && qi >= 0) {
    gp(age.buf[B_CARRY_W])[((size_t)(we >> 1) * age.npub + qi) * 2 + (we & 1)] = acc;
    gp(age.buf[B_CARRY_X])[((size_t)(we >> 1) * age.npub + qi) * 2 + (we & 1)] = xe_;
  }
  if (wls < 3) { Ex[wls * 4 * R + we] = acc; Ex[3 * 4 * R + wls * 4 * R + we] = xe_; }
  WSYNC();
  if (pv && we == 0) {
    double ww[4 * R], xx[4 * R];
#pragma unroll
    for (int i = 0; i < 4 * R; ++i) { ww[i] = Ex[wls * 4 * R + i]; xx[i] = Ex[3 * 4 * R + wls * 4 * R + i]; }
    tangent_inplace<R>(xx, ww);
    double *Gn = age.buf[B_CARRY_G] + fd_pos_off<R>(age.fe_ord, pw);
#pragma unroll
    for (int i = 0; i < 4 * R; ++i) gp(Gn)[i] = ww[i];
  }
}

// k_fd_partial: P for the agent sel(0) -- the streamers of k_step_fd, expression for expression: the first M0 chunks of its M
// against the private rows of its carried gradient, the partial sums of every workgroup into pacc_out
template <int R, int M0>
__global__ __launch_bounds__(256) void k_fd_partial(const AgentDev *__restrict__ agents, int d, double *__restrict__ pacc_out) {
  const AgentDev &agd = agents[d];
  const int hb = (int)blockIdx.x;
  const int bx = (hb % 8) * ((int)gridDim.x / 8) + hb / 8;
  const int tid = threadIdx.x;
  const int N4d = agd.N4;
  if (bx >= (N4d + 7) / 8) return;
  __shared__ double vs[M0 * 64 * R];
  const int cg = (tid >> 5) & 7, kl = tid & 31;
  const int cold = 8 * bx + cg;
  const double *Md = agd.M + (size_t)((cold < N4d) ? cold : 0) * N4d;
  constexpr int NGN = (M0 * 64 * R / 2 + 255) / 256;
  double2 gn[NGN];
#pragma unroll
  for (int u = 0; u < NGN; ++u) gn[u] = ld2(agd.buf[B_CARRY_G] + min(2 * (tid + 256 * u), M0 * 64 * R - 2));
  double2 mn[M0];
#pragma unroll
  for (int i = 0; i < M0; ++i) mn[i] = ld2_nt(Md + min(2 * kl + 64 * (int)agd.fe_ord[i], N4d - 2));
#pragma unroll
  for (int u = 0; u < NGN; ++u) {
    const int tt = 2 * (tid + 256 * u);
    if (tt < M0 * 64 * R) *reinterpret_cast<double2 *>(&vs[tt]) = gn[u];
  }
  lds_barrier();
  double acc[R];
#pragma unroll
  for (int a = 0; a < R; ++a) acc[a] = 0;
#pragma unroll
  for (int i = 0; i < M0; ++i) {
    const int k = 2 * kl + 64 * i;
    double wv[2 * R];
#pragma unroll
    for (int q = 0; q < R; ++q) {
      const double2 t2 = *reinterpret_cast<const double2 *>(&vs[k * R + 2 * q]);
      wv[2 * q] = t2.x; wv[2 * q + 1] = t2.y;
    }
#pragma unroll
    for (int a = 0; a < R; ++a) acc[a] = __builtin_fma(wv[R + a], mn[i].y, __builtin_fma(wv[a], mn[i].x, acc[a]));
  }
#pragma unroll
  for (int a = 0; a < R; ++a) gp(pacc_out)[((size_t)bx * R + a) * 256 + tid] = acc[a];
}

// the deep-carried form needs: every agent's first M0 chunks private, its public poses on two waves (<= 128), its shared
// edges on two waves' two slots (<= FE_MAX_EDGES, all co-resident: fe_code_ok), its rows in the lane-ordered copy
int step_fd_pick_m0(int min_private_chunks) {
  // (fewer private chunks: the waves of the chain would carry too much of the stream.  Measured, round 6: M0 = 20 spills 14
  // registers at r = 5 and runs 15.7 us per launch on sphere2500 / 5 -- slower than round 5's form (14.3); M0 = 16 spills 35:
  // 0.0182 ms per iteration on sphere2500 / 6 against 0.0142)
  const int want[] = {24};
  for (int m : want) if (min_private_chunks >= m) return m;
  return 0;
}

void launch_fd_prime(const LaunchCtx &c, int s0, int s1, int s2, int max_n, int num_robots, int restart_interval, const NestState *nest_src) {
  DPGO_DISPATCH_R(c.r, hipLaunchKernelGGL((k_fd_prime<R>), dim3((max_n + 63) / 64, 3), dim3(64), 0, c.stream, c.agents, s0, s1, s2,
                                          num_robots, restart_interval, nest_src));
}

// what a run opens with behind k_fd_prime: the row products of sel(0) and sel(1), then the private partial sums of sel(0)
void launch_fd_open(const LaunchCtx &c, int m0, int s0, int s1, double *pacc_out) {
  int nblk_all = 0;
  for (int k = 0; k < c.num_agents; ++k) nblk_all = std::max(nblk_all, (c.host_agents[k].N4 + 7) / 8);
  const int gridp = ((c.host_agents[s0].N4 + 7) / 8 + 7) / 8 * 8;
  if (m0 != 24) return;
  switch (c.r) {
    case 3: hipLaunchKernelGGL((k_fd_rows<3>), dim3(nblk_all, 2), dim3(64), 0, c.stream, c.agents, s0, s1, nblk_all);
            hipLaunchKernelGGL((k_fd_partial<3, 24>), dim3(gridp), dim3(256), 0, c.stream, c.agents, s0, pacc_out); break;
    case 4: hipLaunchKernelGGL((k_fd_rows<4>), dim3(nblk_all, 2), dim3(64), 0, c.stream, c.agents, s0, s1, nblk_all);
            hipLaunchKernelGGL((k_fd_partial<4, 24>), dim3(gridp), dim3(256), 0, c.stream, c.agents, s0, pacc_out); break;
    case 5: hipLaunchKernelGGL((k_fd_rows<5>), dim3(nblk_all, 2), dim3(64), 0, c.stream, c.agents, s0, s1, nblk_all);
            hipLaunchKernelGGL((k_fd_partial<5, 24>), dim3(gridp), dim3(256), 0, c.stream, c.agents, s0, pacc_out); break;
    default: break;
  }
}

// the head of a launch (step_head.h) can stand for this agent's descriptor at rank r: its fields fit their widths, its work
// vectors are one allocation (every flag and parity the launches use fits by construction)
bool step_fd_head_ok(const AgentDev &d, int r, int m0) {
  FdHead hd;
  return fd_head_build(hd, d.buf, NBUF, r, d.n, d.N4, d.npub, d.nshared, d.M, d.fe_coef, d.fe_ord, m0, 1, FD_HEAD_FLAGS_MAX, nullptr,
                       (d.N4 + 7) / 8);
}

// sel .. : agents c, d, e, f of the head of the file (d, e, f: any valid agent where the flag is off)
void launch_step_fd(const LaunchCtx &c, int m0, int sel, int next_sel, int next2_sel, int next3_sel, double step, int num_robots,
                    int restart_interval, const NestState *nest_src, NestState *nest_dst, int parity, int flags,
                    const double *pacc_in, double *pacc_out) {
  const AgentDev &d = c.host_agents[sel], &dd = c.host_agents[next_sel], &de = c.host_agents[next2_sel];
  int nblk_all = 0;
  for (int k = 0; k < c.num_agents; ++k) nblk_all = std::max(nblk_all, (c.host_agents[k].N4 + 7) / 8);
  const int grid = (nblk_all + 7) / 8 * 8;
  FdArgs fa = {};
  FeBases &fb = fa.fb;
  FdNext &nx = fa.nx;
  for (int k = 0; k < c.num_agents && k < LOOKAHEAD_MAX_AGENTS; ++k) { fb.ybase[k] = c.host_agents[k].buf[B_Y]; fb.npose[k] = c.host_agents[k].n; fb.part[k] = c.host_agents[k].part; }
  nx.Md = dd.M; nx.N4d = dd.N4; nx.nblk_d = (dd.N4 + 7) / 8; nx.Gd = dd.buf[B_CARRY_G];
  for (int i = 0; i < 32; ++i) { nx.ord_d[i] = dd.fe_ord[i]; nx.ord_e[i] = de.fe_ord[i]; }
  nx.n_e = de.n; nx.soa_w_e = de.soa_w; nx.npub_e = de.npub; nx.soa_col_e = de.soa_col; nx.soa_val_e = de.soa_val;
  nx.pub_index_e = de.pub_index; nx.Ye = de.buf[B_CARRY_Y]; nx.We = de.buf[B_CARRY_W]; nx.Xe = de.buf[B_CARRY_X]; nx.Ge = de.buf[B_CARRY_G];
  fa.ag = d;
  fa.team = c.team; fa.nest_src = nest_src; fa.nest_dst = nest_dst; fa.pacc_out = pacc_out; fa.step = step;
  fa.sel = sel; fa.next_sel = next_sel; fa.next3_sel = next3_sel; fa.num_robots = num_robots;
  fa.restart_interval = restart_interval; fa.num_agents = c.num_agents;
  // (a team takes this form only where every agent's head stands for its descriptor: step_fd_head_ok, fe_deep_m0)
  FdHead hd;
  if (!fd_head_build(hd, d.buf, NBUF, c.r, d.n, d.N4, d.npub, d.nshared, d.M, d.fe_coef, d.fe_ord, m0, parity, flags, pacc_in, nblk_all))
    return;
#define FD_LAUNCH(RR, MM)                                                                                                    \
  hipLaunchKernelGGL((k_step_fd<RR, MM>), dim3(grid), dim3(512), 0, c.stream, hd.buf0, hd.M, hd.pacc_in, hd.fe_coef, hd.np, \
                     hd.sf, hd.ord_lo, hd.ord_hi, hd.nblk_all, fa)
#define FD_LAUNCH_M(RR)                                   \
  switch (m0) {                                           \
    case 24: FD_LAUNCH(RR, 24); break;                    \
    default: break;                                       \
  }
  switch (c.r) {
    case 3: FD_LAUNCH_M(3); break;
    case 4: FD_LAUNCH_M(4); break;
    case 5: FD_LAUNCH_M(5); break;
    default: break;
  }
#undef FD_LAUNCH_M
#undef FD_LAUNCH
}

}  // namespace dpgo
