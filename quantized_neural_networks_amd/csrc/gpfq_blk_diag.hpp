// Diagnostic switches of gpfq_blk.hip -- included ONLY by diagnostic builds (-DGPFQ_BLK_DIAG; never the shipped library):
//   -DGPFQ_BLK_STAMPS    in-kernel phase stamps (s_memtime) of the sweep wavefronts and the decision wavefront of workgroup 0, accumulated
//                        per slot and left in the unused row-statistics area behind the call's counter block (tools/pipe_probe.py prints them)
//   -DGPFQ_BLK_NO_MFMA   phase D (the block dot products) on the vector unit in every shape: the A/B of round 4's matrix form
//   -DGPFQ_BLK_NO_FUSED  matrix-unit phase D as a phase of its own behind the updates: round 4's first form
//   -DGPFQ_BLK_TOP3=n    which slot-top pieces of the symmetric eleven-wavefront shapes go out from inside the pair loop (kTop3Ship in
//                        gpfq_blk.hip is the shipped set): bit 0 the header piece, bit 1 the weight piece; 0 = both at the top of the slot
//   -DGPFQ_BLK_PK_AHEAD=n  the pair loop of the eight-group shapes (kPkAheadShip in gpfq_blk.hip is the shipped set): bit 0 operand rows two
//                        pair-steps ahead, bit 1 the next pair-step's float32 products among this one's conversions and additions; 0 = neither
//   -DGPFQ_BLK_PRIO=n    the issue priorities of the sweep wavefronts in the eight-group shapes (kPrioShip in gpfq_blk.hip is the shipped
//                        setting): bits 0-1 the classic form, bits 2-3 the cluster slices; of a form's two bits the low one raises the slot
//                        top's level in front of the slot's barrier, the high one staggers the level drops by the wavefront's age (kPrioSched)
//   -DGPFQ_BLK_OWN_ROWS=n  the record tiles of the eight-group shapes (kOwnRowsShip in gpfq_blk.hip is the shipped setting; the switch is read
//                        there, host and device): bits 0-1 the classic form, bits 2-3 the cluster slices; of a form's two bits the low one
//                        takes the wavefront-major tiles, the high one requests a slot's tile-sourced rows in front of its barrier
// The marginal-cost experiments of rounds 4-5 (every matrix / vector / LDS / DMA instruction issued twice, the barrier removed, pair splits
// from the environment, the flush forced to one side) were removed in round 6; their numbers are in profiles/r04 and profiles/r05, their
// code in the history (commit 1050215 and before).
#pragma once

#ifdef GPFQ_BLK_NO_MFMA
constexpr bool kNoMfmaD = true;
#else
constexpr bool kNoMfmaD = false;
#endif
#ifdef GPFQ_BLK_NO_FUSED
constexpr bool kNoFused = true;
#else
constexpr bool kNoFused = false;
#endif
#ifdef GPFQ_BLK_TOP3
constexpr int kTop3 = GPFQ_BLK_TOP3;
#else
constexpr int kTop3 = kTop3Ship;
#endif
#ifdef GPFQ_BLK_PK_AHEAD
constexpr int kPkAhead = GPFQ_BLK_PK_AHEAD;
#else
constexpr int kPkAhead = kPkAheadShip;
#endif

#ifdef GPFQ_BLK_PRIO
constexpr int kPrio = GPFQ_BLK_PRIO;
#else
constexpr int kPrio = kPrioShip;
#endif

#ifdef GPFQ_BLK_STAMPS
#define STAMP(var) do { __builtin_amdgcn_sched_barrier(0); var = __builtin_amdgcn_s_memtime(); __builtin_amdgcn_sched_barrier(0); } while (0)
#define STAMP_DO(...) __VA_ARGS__
#else
#define STAMP(var) do { } while (0)
#define STAMP_DO(...)
#endif
