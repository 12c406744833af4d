// lin_common.h -- constants shared by the kernels and the host code of
// jh_lin.hip (included there first): the counter block's words, the flag bits,
// the takeover's handshake values.
#pragma once

namespace {

// The per-call counter block q (device, int32 words; 64-bit counters take two
// words, low word first): queues, list lengths, flags, probe and entry
// counters of the phases. The whole layout:
//    0      Q_QUEUE       phase 1's key queue; then the BFS's (the race, :linear) or k_lin_wg's (tuning mode)
//    1      Q_DEFER       deferred keys, all
//    2      Q_FLAGS       the QF_* bits below
//    3      Q_UNRES       keys the BFS gave up (its unresolved list's length)
//    4-5    Q_PROBES_P1   phase 1's memo probes
//    6      Q_P2_QUEUE    phase 2's LEAN queue
//    7      Q_WIDE_QUEUE  phase 2's WIDE queue
//    8-9    Q_PROBES_SEQ  phase 2's memo probes
//   10-11   Q_BUMP        bytes taken from the tables arena (k_key_tables)
//   12      Q_N_LIST      phase 1's LEAN keys
//   13      Q_N_LIST_W    phase 1's WIDE keys
//   14      Q_P1W_QUEUE   the queue of phase 1's WIDE kernel
//   16      Q_DEFER3      LEAN keys handed to phase 3
//   17      Q_P3_QUEUE_FEW, 18 Q_P3_QUEUE   phase 3's queues (few keys: k_lin_seq; many: k_lin_seq3)
//   19      Q_N_LIST_X    keys with windows of 65-256 members
//   20      Q_P3W_QUEUE   phase 3's WIDE queue
//   21      Q_XW_QUEUE    k_lin_xw's queue
//   22-23   Q_PROBES_XW   k_lin_xw's probes
//   24-25   Q_ENT_ALL     history entries of the deferred keys
//   26-27   Q_XW_MAX      largest k_lin_xw table of a key, bytes
//   28      Q_SEQ_EXIT    sequential waves that have left their queue (the helpers wait for it)
//   29      Q_DEFER_L, 30 Q_DEFER_W, 31 Q_DEFER3W   deferred LEAN / WIDE keys, WIDE keys handed to phase 3
//   32-37   Q_PROBES_HELP, Q_PROBES_P3, Q_PROBES_WIDE
//   40-45   Q_ENT_LEAN, Q_ENT_WIDE, Q_ENT_XW   entries of each list's keys
//   46-49   Q_T_WIDE      first WIDE wave start, last end (s_memrealtime; a span: start at +0, end at +Q_T_END)
//   64      Q_P1_DONE, 65 Q_SEQ_WAVES, 66 Q_BFS_QUEUE   the streaming pass
//   68-83   Q_T_BFS, Q_T_LEAN, Q_T_XW, Q_T_P1   spans, four words each
//   84-85   Q_ENT_P3
//   88-89   Q_RS_USED, 90 Q_RS_PUBLISHED, 91 Q_RS_TAKEOVERS
//   92      Q_MAINS
//   93      Q_BFS_PICKS   keys the BFS took by their stall (round 8)
//   96-97   Q_SPEC, 98 Q_SPEC_MERGES, 99 Q_SPEC_JOBS, 100 Q_SPEC_DEAD
constexpr int Q_WORDS = 104;
constexpr int Q_QUEUE = 0, Q_DEFER = 1, Q_FLAGS = 2, Q_UNRES = 3, Q_PROBES_P1 = 4;
constexpr int Q_P2_QUEUE = 6, Q_WIDE_QUEUE = 7, Q_PROBES_SEQ = 8, Q_BUMP = 10;
constexpr int Q_N_LIST = 12, Q_N_LIST_W = 13, Q_P1W_QUEUE = 14;
constexpr int Q_DEFER3 = 16, Q_P3_QUEUE_FEW = 17, Q_P3_QUEUE = 18, Q_N_LIST_X = 19, Q_P3W_QUEUE = 20;
constexpr int Q_XW_QUEUE = 21, Q_PROBES_XW = 22, Q_XW_MAX = 26, Q_SEQ_EXIT = 28;
constexpr int Q_ENT_ALL = 24, Q_DEFER_L = 29, Q_DEFER_W = 30, Q_DEFER3W = 31;
constexpr int Q_PROBES_HELP = 32, Q_PROBES_P3 = 34, Q_PROBES_WIDE = 36;
constexpr int Q_ENT_LEAN = 40, Q_ENT_WIDE = 42, Q_ENT_XW = 44;
constexpr int Q_T_WIDE = 46;        // [46..47] first WIDE wave start, [48..49] last end (s_memrealtime)
constexpr int Q_T_END = 2;          // a span's last-end words, after its first-start words
// the streaming heavy-key pass (round 4): phase 1's finished keys, the LEAN
// sequential waves of both grids, the BFS's queue, and spans (first key taken,
// last wave end; s_memrealtime) of the BFS, the LEAN role, the xw role and phase 1
constexpr int Q_P1_DONE = 64, Q_SEQ_WAVES = 65, Q_BFS_QUEUE = 66;
constexpr int Q_T_BFS = 68, Q_T_LEAN = 72, Q_T_XW = 76, Q_T_P1 = 80;
constexpr int Q_ENT_P3 = 84;        // entries of the LEAN keys restarted in phase 3
constexpr int Q_RS_USED = 88;       // [88..89] resume records' bytes, [90] records published (round 5), [91] takeovers (round 6)
constexpr int Q_RS_PUBLISHED = 90, Q_RS_TAKEOVERS = 91;
constexpr int Q_MAINS = 92;         // round 6: late helpers running a key now
constexpr int Q_BFS_PICKS = 93;     // round 8: keys k_lin_bfs took by their published stall (bfs_pick)
constexpr int Q_SPEC = 96;          // round 6: [96..97] merged nodes, [98] merges, [99] spec jobs, [100] dead results
constexpr int Q_SPEC_MERGES = 98, Q_SPEC_JOBS = 99, Q_SPEC_DEAD = 100;
// bits of the flags word q[Q_FLAGS]: any of them fails the call (JH_EDEVICE)
constexpr int QF_TABLE_OVERFLOW = 2;    // a per-key table exceeded the scratch reservation
constexpr int QF_STACK_OVERFLOW = 4;    // DFS stack overflow
// the workgroup engine's watchdogs (no kernel sets 16, 32 or 256 today; the host still reports them)
constexpr int QF_LOST_ITEM = 16, QF_IDLE_ENUM = 32, QF_FULL_SET = 64, QF_STEP_LIMIT = 128;
constexpr int QF_BAD_WINDOW = 256;
constexpr int QF_STREAM_WAIT = 512;     // stream_key waited past STREAM_WATCHDOG
constexpr int QF_WG_WATCHDOGS = 0x1F0;  // 16 .. 256: the [jh-acc] traces explain these
constexpr int QF_WATCHDOGS = 0x3F0;     // 16 .. 512

// the takeover's handshake (DfsArgs::handoff), and dfs_lean's verdict for a handed-over search
constexpr int V_HANDED = -9;            // dfs_lean: saved for a takeover, continue from the record
constexpr int32_t HO_NONE = 0, HO_ASK = 1, HO_DONE = 2, HO_REFUSED = 3, HO_WITHDRAWN = 4, HO_SAVING = 5;

}  // namespace
