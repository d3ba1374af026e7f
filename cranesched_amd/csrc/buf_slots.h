// The slots of cns_engine's per-feature device buffer sets: one enum per set, its *_COUNT sizes the array.
#pragma once

// JobTable::raw (engine.hip, job_table.inc): the caller's job arrays as uploaded, then what the host pass adds; k_pack_jobs reads them all
enum { JR_LIMIT = 0, JR_NCPU, JR_NMEM, JR_TCPU, JR_TMEM, JR_K, JR_NTASKS, JR_TMIN, JR_TMAX, JR_EXCL, JR_GTOT, JR_GSPEC, JR_INCL_OFF, JR_EXCL_OFF,
       JR_PLACE_OFF, JR_GROUPED, JR_COUNT };

// cns_engine::d_prio (priority_host.inc)
enum { PR_SUBMIT = 0, PR_QOS, PR_PART, PR_NODENUM, PR_CPU, PR_MEM, PR_ACCT, PR_CACHED,                                          // jobs: pending
       PR_RSTART, PR_RQOS, PR_RPART, PR_RNODENUM, PR_RCPU, PR_RMEM, PR_RACCT,                                                   // jobs: running
       PR_ACCOFF, PR_ACCJOBS, PR_PRESENT, PR_BOUNDS, PR_ACCVAL,                                                                 // tables
       PR_PRIO, PR_K0, PR_K1, PR_V0, PR_V1, PR_HIST, PR_TERMS, PR_COUNT };                                                      // scratch

// cns_engine::d_lim (limits_host.inc)
enum { LM_LIM = 0, LM_QFLAGS, LM_PARENT, LM_LEVEL, LM_UPL, LM_APL, LM_USAGE0, LM_EXISTS0, LM_USAGE, LM_EXISTS,                  // tables
       LM_SEL, LM_USER, LM_UA, LM_ACCT, LM_QOS, LM_PART, LM_TL, LM_SKIP, LM_PLACEOFF,                                           // jobs
       LM_BLKCNT, LM_BLKOFF, LM_CTR, LM_RECADD, LM_RECC, LM_RECL, LM_RECEN, LM_RECJOB, LM_RECMETA, LM_OUT, LM_COUNT };          // scratch

// cns_engine::d_limpar (limits_host.inc): the parallel pass of the admission
enum { LP_K0 = 0, LP_K1, LP_V0, LP_V1, LP_HIST,                                                                                 // scratch: the sort
       LP_SKEY, LP_SK, LP_SL, LP_SEN, LP_SSLOT, LP_SADD,                                                                        // scratch: the sorted items
       LP_STATE, LP_FLAGS, LP_JOBKEY, LP_TAILS, LP_HEADS, LP_CARRY, LP_COUNT };                                                 // scratch: the rounds

// cns_engine::d_step (steps_call.inc)
enum { ST_NODEOFF = 0, ST_NODEIDX, ST_AVAIL, ST_STEPOFF, ST_STEPS, ST_INCL, ST_EXCL,                                            // jobs
       ST_SCHEDULED, ST_ONODE, ST_ONT, ST_OALLOC, ST_TNODE, ST_TALLOC, ST_COUNT };                                              // results

// cns_engine::d_pb (probe_host.inc): what the probes need besides their job table (cns_engine::pt)
enum { PB_PARAMS = 0, PB_PART, PB_CTR, PB_HEAP, PB_FAULT, PB_COUNT };

// cns_engine::d_rq (resvq_host.inc)
enum { RQ_LATEST = 0, RQ_RVOFF, RQ_RVST, RQ_RVED, RQ_RAW_END, RQ_RAW_OFF, RQ_RAW_NODE,                              // state
       RQ_START, RQ_DUR, RQ_K, RQ_FLAGS, RQ_CANDOFF, RQ_CAND, RQ_CHOFF,                                              // queries
       RQ_EVOFF, RQ_SEGOFF, RQ_KA, RQ_KB, RQ_KC, RQ_VA, RQ_VB, RQ_SORTED, RQ_HIST, RQ_BEST,                              // earliest mode
       RQ_CODE, RQ_CHOSEN, RQ_STATUS, RQ_OSTART, RQ_NFREE, RQ_COUNT };                                               // results

// cns_engine::d_vd (valid_host.inc)
enum { VD_NCPU = 0, VD_NMEM, VD_NGRES, VD_NUNSUP, VD_NODE, VD_POFF, VD_PNODES, VD_TOTAL, VD_RVOFF, VD_RVNODES,              // tables
       VD_JNCPU, VD_JNMEM, VD_JTCPU, VD_JTMEM, VD_JK, VD_JNT, VD_JGT, VD_JGS, VD_JRSV, VD_IOFF, VD_INCL, VD_EOFF, VD_EXCL,    // jobs
       VD_ORDER, VD_CHUNKS, VD_CODE, VD_ELIG, VD_COUNT };                                                                     // the call

// cns_engine::d_cc (commit_host.inc)
enum { CC_CHANGE = 0, CC_EVTIME, CC_EVOFF, CC_EVNODES, CC_SLOT, CC_AREX, CC_AREND, CC_AROFF, CC_ARNODES,   // events
       CC_LIMIT, CC_RESV, CC_GONE, CC_PREOFF, CC_PRE, CC_ALIVE,                                             // jobs
       CC_CODE, CC_COUNTS, CC_COUNT };                                                                      // results

// cns_engine::d_sub (submit_host.inc)
enum { SB_QOS = 0, SB_PL, SB_PARENT, SB_UPL, SB_APL, SB_UQ, SB_AQ, SB_G, SB_ST_SET, SB_ST,                                    // tables
       SB_JPART, SB_JTL, SB_JNCPU, SB_JNMEM, SB_JTCPU, SB_JTMEM, SB_JK, SB_JNT, SB_JGT, SB_JGS,                                // jobs
       SB_KUSER, SB_KUA, SB_KACCT, SB_KQOS, SB_KCOUNT, SB_KSKIP,                                                                // keys
       SB_PRE, SB_STATE, SB_STAT, SB_COND, SB_IKEY, SB_ITHR, SB_CODE, SB_TLO, SB_CTR,                                           // per job
       SB_SK0, SB_SK1, SB_SV0, SB_SV1, SB_HIST, SB_SKEY, SB_SITEM, SB_SADD, SB_VAL, SB_TAILS, SB_HEADS, SB_CARRY, SB_COUNT };   // the parallel pass

// cns_engine::d_use (usage_host.inc)
enum { US_PARENT = 0, US_TAB_SET, US_TAB_CUR, US_TAB_WORK,                                                                        // tables
       US_JUSER, US_JUA, US_JACCT, US_JQOS, US_JPART, US_JCPU, US_JMEM, US_JWALL, US_JJOBS, US_JSUB, US_JNT, US_JCC, US_JSKIP,     // rows
       US_DELTA, US_MASK, US_CTR, US_SK0, US_SK1, US_SV0, US_SV1, US_HIST, US_SKEY, US_SITEM,                                     // items
       US_TAILS, US_TFLAGS, US_CARRY, US_CFLAGS, US_COUNT };                                                                      // the scan

// cns_engine::d_gate (gate_host.inc)
enum { GT_JOBID = 0, GT_HELD, GT_BEGIN, GT_ISOR, GT_READY, GT_DEPOFF, GT_DEPJOB, GT_DELAY, GT_AP, GT_APFLAGS, GT_APDEAD, GT_APRUN, GT_APLIM,   // jobs
       GT_EVDEPENDENT, GT_EVDEPENDEE, GT_EVSEC, GT_FIRST,                                                                                     // events
       GT_CODE, GT_READYOUT, GT_ERASED, GT_WAVES, GT_TOTAL, GT_PENDING, GT_COUNTS, GT_COUNT };                                                // results

// cns_engine::d_rl (running_host.inc)
enum { RL_ID = 0, RL_END, RL_RESV, RL_OFF, RL_NODE, RL_RES,                                                 // the ledger
       RL_WID, RL_WEND, RL_WRESV, RL_WOFF, RL_WNODE, RL_WRES,                                               // the call's copy of it
       RL_RET, RL_FOUND, RL_JID, RL_ADMIT, RL_JRESV,                                                        // the call's lists
       RL_WROWS0, RL_WENTS0, RL_WROWS1, RL_WENTS1, RL_TOT, RL_NSOFF, RL_NS, RL_WEXP,                        // counts, the node -> slots CSR
       RL_K0, RL_K1, RL_V0, RL_V1, RL_HIST, RL_RNOFF, RL_RNEND, RL_RNRES, RL_FLAG,                          // pairs, the per-slot tables
       RL_AMID, RL_AMEND, RL_COUNT };                                                                       // cns_running_amend_ends: the sorted ids, their ends

// cns_engine::d_rp (running_preempt_host.inc): the sorted (slot, allocation) pairs of the last rebuild, the index built from them,
// the call's lists and tables
enum { RP_KEYS = 0, RP_VALS, RP_ENTJOB, RP_ENTSLOT, RP_K0, RP_K1, RP_V0, RP_V1, RP_HIST, RP_RJOFF, RP_RJENT,   // per rebuild
       RP_GIVEN, RP_SET, RP_FOUND, RP_FLAG, RP_RJPRE, RP_RJEND, RP_ENTEND, RP_COUNT };                         // per call

// cns_engine::d_ra (running_host.inc, running_attrs_host.inc): the attribute columns beside the ledger, the call's copy of them, what a
// cycle boundary needs to carry them, the per-row sums, the running side of cns_priority_order_resident
enum { RA_START = 0, RA_QOS, RA_QPRIO, RA_PART, RA_ACCT,                                                    // the columns
       RA_WSTART, RA_WQOS, RA_WQPRIO, RA_WPART, RA_WACCT,                                                   // the call's copy of them
       RA_ORIGIN, RA_QQOS, RA_QQPRIO, RA_QPART, RA_QACCT,                                                   // a cycle boundary: where a row came from, the queue's attributes
       RA_NODENUM, RA_CPU, RA_MEM, RA_SUMFLAG,                                                              // per ledger state: the sums, their flag words
       RA_FLAG, RA_K0, RA_K1, RA_V0, RA_V1, RA_HIST, RA_PICK, RA_PICKED, RA_COUNT };                        // per call

// cns_engine::d_pre (engine.hip: a cycle with preemption)
enum { B_QPOFF, B_QP, B_PJQOS, B_PJQP, B_PJPRIO, B_PJREC0, B_PJK, B_PJEND, B_RNJOB, B_ENTSLOT, B_ENTGONE, B_RJQOS, B_RJQP,
       B_RJSTART, B_RJEND, B_RJPRE, B_RJOFF, B_RJENT, B_HEAD, B_RECNEXT, B_RECORIG, B_RECSLOT, B_RECGONE, B_MISC, B_COUNT };
