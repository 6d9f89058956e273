// capi_internal.h -- context and helpers shared by the C-ABI translation units.
#ifndef TRACY_AMD_CAPI_INTERNAL_H
#define TRACY_AMD_CAPI_INTERNAL_H

#include <hip/hip_runtime.h>

#include <atomic>
#include <condition_variable>
#include <deque>
#include <functional>
#include <mutex>
#include <string>
#include <thread>
#include <utility>
#include <vector>

#include "../../include/tracy_hip.h"
#include "assemble_wave.h"
#include "dp_kernels.h"
#include "dp_plan.h"
#include "band16_launch.h"
#include "front.h"

namespace tracyhip {

struct DevBuf {  // grow-only device buffer
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes);
  void release();
};
// `count` elements of T in a grow-only buffer (DevBuf or PinBuf), and the typed pointer to them
template <class Buf, class T>
hipError_t ensure_into(Buf& b, size_t count, T*& p) { const hipError_t e = b.ensure(sizeof(T) * count); p = static_cast<T*>(b.p); return e; }
struct PinBuf {  // grow-only pinned host buffer (descriptor uploads)
  void* p = nullptr;
  size_t cap = 0;
  hipError_t ensure(size_t bytes);
  void release();
};
// Every device buffer a context keeps between calls: tracyhip_ctx::dev[].  One slot, one role; where two roles share a slot the
// second is written as an alias with the reason why the two are never live in one call (DevBuf::ensure frees what it outgrows).
enum CtxDev : int {
  // ---- the generic DP launches (capi.hip run_dp / run_band16 / run_front) and what every pipeline stages through them ----
  DB_DESC,     // PairDesc / per-trace descriptors: uploaded by run_dp, run_ckpt_prefix, the decompose entry points, consensus_run, assemble_run; read by their kernels
  DB_BITS,     // traceback words: written by the traceback sweeps of run_dp / run_band16 and the stream-ordered band stages, read by their walks; LDS spill of breakpoint / allelicFraction
  DB_SCRATCH,  // strip hand-over rows of multi-pass sweeps: written and read inside one run_dp / consensus_run / assemble_run launch
  DB_IN1,      // first payload of a call staged from the host (stage_in): profiles / a1 / signal / peaks; read by that call's kernels
  DB_IN2,      // second payload staged from the host: references / a2 / bcpos
  DB_CODES,    // encoded reference codes with kCodePad on both sides: written by the encode kernels (ensure_codes), read by every MODE_QP / band sweep
  DB_SCORES,   // staged score results of tracyhip_score / align / band16 and score_final of align_traces (no_stream), host arrays only
  DB_OPS,      // staged traceback strings of the same calls; the ops uploaded by tracyhip_alignment_rows
  DB_OPS_OFF,  // offsets of the traceback strings, uploaded per call, read by the walks
  DB_OPS_LEN,  // staged lengths of the traceback strings
  DB_ERR,      // kErrBytes of error / verdict words: cleared by the host, set by kernels, read back once per stage
  DB_ROWS0,    // alignment rows: staged in by the decompose entry points and trim_reference_slice, written by tracyhip_alignment_rows
  DB_ROWS1,    // the second row of each pair, as DB_ROWS0
  DB_SPECIAL,  // one byte per 256 code bytes: set by the encoders (ensure_codes), read by the compact 16-bit sweeps
  DB_ENDS,     // ends of the preliminary alignments + scratch of that stage: OrientRun::prelim; staged ends of tracyhip_band16
  DB_CKPT,     // wavefront checkpoints: written by the DP_CKPT sweeps of OrientRun, read by its DP_BAND traceback
  DB_LASTROW,  // last-row values / kept prefix rows: written by the DP_CKPT and prefix sweeps, read by row_m_end, the pruned sweeps and both stream-ordered calls
  DB_BAND,     // band traceback words of run_dp(DP_BAND); scan state of decompose_kernel_global
  DB_B16TAB_ALLELE0,  // substitution tables (band16.h) of allele k = 0: build_b16_tables in decompose / tracyhip_band16, read by the band kernels
  DB_B16TAB_ALLELE1,  // the same for allele k = 1 of decompose (indexed DB_B16TAB_ALLELE0 + k)
  DB_B16TAB_PROFILE,  // substitution tables of the full trace profiles: align_traces and decompose_traces in both forms
  DB_B16DESC,  // B16TableDesc list of build_b16_tables, read by b16_table_kernel
  DB_FRONT,    // descriptors / pairs / results of the pruned orientation sweep: run_front
  DB_PRE,      // descriptors of its prefix launch over string x code pairs: run_prefix_keep_cq
  DB_STREAM,   // the Arena of the stream-ordered pipelines (stream.hip): everything they keep between their stages
  DB_AFTAB,    // allelicFraction grid enumeration, uploaded once (aftab_ready), read by the af kernels
  DB_AFSCRATCH,  // af_prepare_kernel -> af_search_kernel: tp, class bytes, headers
  DB_DECLUT,   // decompose_wave.h class table, uploaded once (declut_ready)
  DB_DECTODO,  // per trace "left to decompose_kernel": written by decompose_wave_kernel, read by decompose_kernel
  // ---- scratch of the host-planned pipelines and the single-step entry points (one call at a time per context) ----
  DB_ORIENT_SC2,    // both orientation scores per trace: written by OrientRun's sweeps (align_traces no_stream), read back by fetch_scores
  DB_PRELIM_OPS,    // ops of the preliminary alignment: written by OrientRun::prelim for AlignRun, read by trim_kernel
  DB_PRELIM_OFF,    // their offsets: uploaded by AlignRun::orient
  DB_PRELIM_LEN,    // their lengths: written with the ops, read by trim_kernel
  DB_PRELIM_SCORE,  // preliminary scores: written by OrientRun::prelim, copied out by AlignRun::results
  DB_TRIMREC,       // TrimRec per trace: written by the trim kernels of AlignRun::trim and tracyhip_trim_reference_slice, read back at once
  DB_TRIM_IN,       // reference lengths + strands: uploaded by AlignRun::trim, read by its trim kernel
  DB_VOTE,          // vote block of OrientRun::vote_block: descriptors up, votes / bounds written by kmer_vote / rowmax_rest, read by the sweeps and fetch_vote_block
  // build_problem runs in tracyhip_score / tracyhip_align only, never inside a pipeline: no OrientRun is alive beside it
  DB_ROW4DESC = DB_ORIENT_SC2,  // ProfSeq list of the profile x profile column classes: build_problem
  // the decompose entry points below are calls of their own; each waits for its stream before it returns
  DB_BP_STAGE = DB_ORIENT_SC2,         // staged tracyhip_breakpoint array: find_breakpoint (out), find_homozygous_breakpoint (in / out), decompose_alleles (in)
  DB_HZ_STATUS_STAGE = DB_PRELIM_OPS,  // staged status of find_homozygous_breakpoint
  DB_PRIMARY_STAGE = DB_PRELIM_OPS,    // staged primary basecalls: decompose_alleles (in / out), secondary_decomposed, allelic_fraction (in); never with DB_HZ_STATUS_STAGE
  DB_SECONDARY_STAGE = DB_PRELIM_OFF,  // staged secondary basecalls / secdecomp of the same three calls
  DB_DCP_INDEL_STAGE = DB_PRELIM_LEN,  // staged dcp_indel table of decompose_alleles
  DB_BC_RESULT_STAGE = DB_PRELIM_LEN,  // staged result of secondary_decomposed (secdecomp) / allelic_fraction (fractions): one of the three per call
  DB_DCP_ERR_STAGE = DB_PRELIM_SCORE,  // staged dcp_err table of decompose_alleles
  DB_DECOMP_STATUS_STAGE = DB_TRIMREC, // staged status of decompose_alleles (takes a caller's peak-free basecalls: bc_descs does not run)
  DB_PEAKS = DB_TRIMREC,               // peak table built by bc_descs for secondary_decomposed / allelic_fraction, read by their one kernel; neither stages a status
  // AlignRun::trim ends on ctx_sync: its trim kernel has read DB_TRIM_IN before final_alignment writes here
  DB_FINAL_TOP = DB_TRIM_IN,  // RowMaxDesc + bound tops of the banded final alignments: AlignRun::final_alignment
  // prelim() runs behind the wait of fetch_scores / sync_verdict, and ck.d_votes is cleared before it: no sweep or copy still reads a vote block
  DB_BAND_SCORES = DB_VOTE,   // scores of the banded preliminary tracebacks: OrientRun::prelim (tb16_path)
  // tracyhip_pack_ragged is a call of its own and waits for its stream
  DB_PACK_SCAN = DB_VOTE,     // scan scratch of pack.hip
  // ---- tracyhip_decompose_traces (no_stream): DecomposeRun hands these out in order (buf()), fourteen fixed roles first ----
  DB_PIPE0 = DB_VOTE + 1,
  DB_PIPE_END = DB_PIPE0 + 64,
  DB_SEED_TRACES = DB_PIPE_END,  // tracyhip_seed_traces (seed.hip): per-trace inputs up, results of seed_traces_kernel back
  DB_SEED_CONS,     // consensus staged from the host, read by the seeding kernels
  DB_SEED_WINDOWS,  // reference windows written by the seeding kernels for a host caller, copied back
  DB_SEED_SPILL,    // option seed_spill: descriptors (uploaded) and counting tables of the traces of one spill launch, cleared and read by seed_spill_kernel
  DB_BCALL_TRACES,   // tracyhip_basecall_traces (basecall.hip): per-trace inputs up, per-trace results back
  DB_BCALL_SCRATCH,  // working words of basecall_kernel
  DB_BCALL_SIGNAL,   // signal staged from the host
  DB_BCALL_POS,      // basecall positions staged from the host
  DB_BCALL_PAY,      // payload results staged for a host caller
  // ---- tracyhip_consensus_traces (consensus.hip consensus_run) ----
  CB_A2,        // both strands of the second profile of each pair: copied in, the reverse written by prof_revcomp_kernel; read by the sweeps
  CB_SEQS,      // ProfSeq list, uploaded
  CB_CLASS,     // "row 4 is all zero" byte per profile: written by prof_classify_kernel, read back
  CB_COLCLASS,  // column classes of both strands: written by prof_classify_kernel, read by the screened score sweeps
  CB_SC2,       // both strand scores per pair, read back
  CB_OPS,       // traceback strings: written by the traceback walk, read by consensus_kernel
  CB_OFF,       // their offsets, uploaded
  CB_PAIR,      // per-pair results staged for a host caller
  CB_PAY,       // payload results (consensus, qualities, ...) staged for a host caller
  CB_FIX,       // ConsFixup list + its counter: written by consensus_kernel, read back
  CB_PATCH,     // ConsPatch list, uploaded for cons_patch_kernel
  CB_GQ,        // gq table of consensus.h, uploaded once (cons_gq_ready)
  // ---- tracyhip_assemble_traces (assemble.hip assemble_run) ----
  AB_TR,        // both strands of every trace profile: copied in, the reverse written by prof_revcomp_kernel; read by the sweeps
  AB_SEQS,      // ProfSeq list, uploaded
  AB_CLASS,     // "row 4 is all zero" byte per trace and reference: written by prof_classify_kernel, read back
  AB_REFCLASS,  // column classes of the references: written by prof_classify_kernel, read by the screened score sweeps
  AB_SC2,       // both strand scores per trace, read back
  AB_OPS,       // traceback string of the current step of every group
  AB_OFF,       // their offsets, uploaded
  AB_LEN,       // their lengths, read back per step
  AB_W0,        // row blocks of the growing alignments, ping
  AB_W1,        // ... pong
  AB_SPAN,      // first / last column of every row
  AB_PROF,      // profile of the alignment so far: written by msa_profile_kernel, read by the next step's sweep
  AB_PCLASS,    // its column classes
  AB_STEP,      // AsmStep + AsmFinal per group, uploaded per step
  AB_PAY,       // payload results staged for a host caller in the caller's layout (GroupOut::bind, for both group calls)
  // ---- tracyhip_denovo_traces (denovo.hip denovo_run) ----
  // a context runs one call at a time, and neither call keeps anything in these between calls: the roles that match share a slot
  DN_PROF = AB_TR,      // [forward | revcomp] of every trace, then the node profiles: both sides of every dynamic program
  DN_SEQS = AB_SEQS,    // ProfSeq list of both strands, uploaded
  DN_CLASS = AB_CLASS,  // "row 4 is all zero" byte per profile, read back
  DN_COLCLASS = AB_PCLASS,  // column classes, indexed like DN_PROF: the inputs by prof_classify_kernel, the nodes by msa_profile_kernel
  DN_TABLE = AB_SC2,    // the strand table T[i][j][oi][oj] of every group, read back
  DN_OPS = AB_OPS,      // traceback strings: one per trace in an overlap round, one per node at a tree height
  DN_OFF = AB_OFF,      // their offsets: uploaded once for the rounds, once per chunk for the tree
  DN_LEN = AB_LEN,      // their lengths, read back per round / height
  DN_ROWS = AB_W0,      // row blocks of the nodes below the roots (the roots write into the caller's rows)
  DN_SPAN = AB_SPAN,    // first / last column of every row of every node
  DN_STEP = AB_STEP,    // AsmStep per node of a height + AsmFinal per group, uploaded per height / chunk
  DN_PAY = AB_PAY,      // results staged for a host caller
  DN_CNT,       // 's' ops of every overlap alignment of a round: written by denovo_count_kernel, read back per round (a slot of its own,
                // and the last enumerator before the next family: the aliases above do not advance the count)
  // ---- tracyhip_call_variants / tracyhip_decompose_variants (variants.hip) ----
  // rows live in DB_ROWS0 / DB_ROWS1 (staged in by the stage, written by the alignment_rows launches of the pipeline)
  VB_DESC,      // VarDesc per trace of a chunk, uploaded; read by variants_kernel
  VB_EVENTS,    // 2 x max_variants VarEvent per resident wave: the two per-allele lists of variants_wave
  VB_LEN,       // column counts of the alignments: uploaded by the stage; the pipeline's copy of a host caller's ops_len[0 | 1]
  VB_PAIRS,     // PairDesc lists of the pipeline's alignment_rows launches, uploaded per chunk
  VB_RCDESC,    // VarRcDesc list of var_revcomp_kernel, uploaded per chunk
  VB_SEQ,       // reverse complements of the trimmed alleles and their slices (reverse traces): both sides of the re-alignments
  VB_OPS,       // op strings of the re-alignments, written by the traceback batch, read by alignment_rows
  VB_OPS_OFF,   // their offsets (the rows of a re-alignment sit at the same offset in the reverse region of DB_ROWS0 / 1), uploaded
  VB_OPS_LEN,   // their lengths, written with the ops, read by alignment_rows and variants_kernel
  VB_IN_PRIMARY,    // a host caller's primary / secdecomp / references / ops[0] / ops[1] of the pipeline, staged in once per call
  VB_IN_SECDECOMP,
  VB_IN_REFS,
  VB_IN_OPS0,
  VB_IN_OPS1,
  VB_OUT_REC,   // records / text / counts + flags staged for a host caller
  VB_OUT_TEXT,
  VB_OUT_N,
  VB_PACK_OFF,  // var_pack_scan_kernel: where every trace's records and text begin in the packed copies
  VB_PACK_REC,  // the used records of every trace back to back: written by var_pack_copy_kernel, copied to the host
  VB_PACK_TEXT, // the used text likewise
  // ---- tracyhip_align_traces with a wildtype-trace reference (wildtype.hip wildtype_run) ----
  WB_ORIENTED,  // caller-oriented jobs: the strand byte of every trace, uploaded; read by wt_decide_kernel (the one slot of its own,
                // before the aliases: they do not advance the count)
  // the same stages as consensus_run over the same kinds of data, and a context runs one call at a time: the roles that match share a slot
  WB_W = CB_A2,          // both strands of every DISTINCT wildtype profile: copied in, the reverse written by prof_revcomp_kernel
  WB_SEQS = CB_SEQS,     // ProfSeq list (traces, then wildtypes), uploaded
  WB_CLASS = CB_CLASS,   // "row 4 is all zero" byte per trace and wildtype, read back
  WB_COLCLASS = CB_COLCLASS,  // column classes of both strands of the wildtypes, read by the screened score sweeps
  WB_SC2 = CB_SC2,       // the strand scores per trace (two, or one for caller-oriented jobs): written by the score sweeps, read by wt_decide_kernel
  WB_OFF = CB_OFF,       // offsets of the op strings / rows, uploaded
  WB_PAIR = CB_PAIR,     // per-trace results staged for a host caller (and score_prelim where the caller wants none)
  WB_PAY = CB_PAY,       // ops / rows0 / rows1 staged for a host caller
  // ---- tracyhip_pad_traces (pad.hip) ----
  PD_TRACES = WB_ORIENTED + 1,  // PadTrace per trace up, PadOut per trace back
  PD_SCRATCH,   // the insert lists of pad_kernel, one region per trace of a chunk
  PD_IN,        // a host caller's chromatograms, basecall arrays and rows of a chunk, staged in
  PD_OUT,       // padded chromatograms and basecall arrays of a chunk staged for a host caller
  // ---- tracyhip_render_traces (render.hip) ----
  DB_RENDER_TRACES,  // RenderTrace per trace up, RenderOut per trace back
  DB_RENDER_TILES,   // bytes (then offset) and aux word of every tile of a chunk: written by render_count_kernel, scanned in place by
                     // render_scan_kernel, read by render_emit_kernel
  DB_RENDER_IN,      // a host caller's chromatograms and basecall arrays of a chunk, staged in
  DB_RENDER_OUT,     // the text of a chunk staged for a host caller
  // ---- tracyhip_read_traces (read.hip) ----
  DB_READ_FILES,     // ReadFile per file up, ReadDesc per file written by read_scan_kernel and brought back
  DB_READ_IN,        // a host caller's file images of a chunk, staged in
  DB_READ_OUT,       // chromatograms and call arrays of a chunk staged for a host caller
  // ---- tracyhip_render_alignments, tracyhip_reference_slices (alntext.hip) ----
  DB_ALNTEXT_DESC,   // AlnDesc per alignment up, AlnOut per alignment back; SliceDesc per slice up
  DB_ALNTEXT_TILES,  // bytes (then offset) and the two letter counts of every tile of a chunk: written by alntext_count_kernel, scanned in
                     // place by alntext_scan_kernel, read by alntext_emit_kernel; behind them the letters of every column tile
                     // (alntext_letters_kernel)
  DB_ALNTEXT_IN,     // a host caller's rows and names of a chunk, staged in; a host caller's references (slices)
  DB_ALNTEXT_OUT,    // the text of a chunk staged for a host caller; the slices staged for a host caller
  // ---- tracyhip_render_decompositions (dcptext.hip) ----
  DB_DCPTEXT_DESC,   // DcpDesc per trace up, DcpOut per trace back
  DB_DCPTEXT_TILES,  // bytes (then offset) and the check word of every tile of a chunk: written by dcptext_count_kernel, scanned in place by
                     // dcptext_scan_kernel, read by dcptext_emit_kernel
  DB_DCPTEXT_IN,     // a host caller's tables, rows, basecalls, variants and names of a chunk, staged in
  DB_DCPTEXT_OUT,    // the text of a chunk staged for a host caller
  DB_COUNT = DB_DCPTEXT_OUT + 1
};
static_assert(DN_CNT + 1 == VB_DESC && VB_PACK_TEXT + 1 == WB_ORIENTED && DN_PAY < DB_COUNT && WB_PAY < DB_COUNT,
              "an alias does not advance the count: every slot of its own comes after the aliases");
// pinned host buffers of a context: tracyhip_ctx::pin[]
enum CtxPin : int {
  PB_DESC,      // descriptor uploads of run_dp and the batch calls
  PB_OFF,       // offset uploads (DB_OPS_OFF, CB_OFF, AB_OFF)
  PB_TMP,       // per-stage uploads of AlignRun and assemble_run
  PB_RES,       // small result read-backs and the vote block's host side
  PB_PRE,       // descriptors of run_prefix_keep_cq
  PB_B16DESC0,  // ring of four B16TableDesc uploads (build_b16_tables, b16_round)
  PB_COUNT = PB_B16DESC0 + 4
};

int set_error(int code, const char* fmt, ...);
// a HIP call inside a function that returns a status of the C ABI: on failure the last error is set and the function returns
#define HIP_TRY(expr)                                                                               \
  do {                                                                                              \
    hipError_t _e = (expr);                                                                         \
    if (_e != hipSuccess)                                                                           \
      return set_error(_e == hipErrorOutOfMemory ? TRACYHIP_ERR_OOM : TRACYHIP_ERR_HIP, "%s failed: %s (%s:%d)", \
                       #expr, hipGetErrorString(_e), __FILE__, __LINE__);                           \
  } while (0)

// Every switch of the library in one place.  Read from the environment ONCE, when a context is created (TRACYHIP_<NAME IN CAPITALS>),
// changed afterwards only through tracyhip_set_option(ctx, "<name>", "<value>"); tracyhip_describe() prints them.  Every one selects
// another exact path (A/B measurements, tests of the fallback tiers); none changes a result.  Lanes inherit their context's.
struct CtxKnobs {
  bool no_stream = false;         // pipelines planned by the host between launches (the pre-round-4 form) instead of stream-ordered
  bool no_narrow = false;         // int32 score kernels instead of the 16-bit sweeps
  bool no_compact = false;        // every 16-bit sweep on the six-code table
  bool no_screen = false;         // profile x profile scores by the full float chain only
  bool no_band = false;           // no checkpointed score pass / band traceback: whole-matrix tracebacks
  bool no_band16 = false;         // no band kernels (band16.h)
  bool no_front = false;          // no pruned sweeps (front.h)
  bool no_prefix = false;         // no prefix bounds (strand by certificate, pruned sweeps)
  bool no_vote = false;           // no k-mer orientation vote
  bool no_origin = false;         // allele-vs-window alignments by full traceback instead of the origin-tracking sweep
  bool no_subwindow = false;      // origin sweeps over the whole window
  bool no_prelim_origin = false;  // preliminary alignment of `tracy align` by band traceback instead of its two ends
  bool no_cq = false;             // string x string by byte compare instead of the query-profile table
  bool no_fused_walk = false;     // a separate walk launch after a traceback sweep
  bool no_quads = false;          // stream-ordered pipelines: narrow bands on sixteen lanes per pair like the rest (band16.h b16_narrow_ok)
  bool no_fork = false;           // stream-ordered pipelines: the launches of a band stage in a row on the call's stream instead of side by side
  bool no_early_tail = false;     // `tracy align`, stream-ordered: no trace's preliminary / final alignment is queued on the voted strand's side stream before the
                                  // other strand's full sweep has confirmed the vote -- every trace takes the pass behind the decision (the order before the early tail)
  bool sweeps_alone = false;      // MEASUREMENT mode of the stream-ordered orientation stage: the voted strand's chain finishes BEFORE the other strand's full sweeps
                                  // start and its prefix cells are credited to the front timer -- TRACYHIP_TIMER_SCORE then times the full sweeps on a device
                                  // of their own (bench.py roofline.dominant_kernel_alone_frac); slower, same results
  bool no_sweep_diag = false;     // the 16-bit query-profile sweeps on values as they are (eight operations per cell) instead of the offset form (six)
  bool no_origin_band = false;    // `tracy decompose`, gotoh(allele, slice): the band d1 +- (g + 1) of every co-optimal path instead of the g + 3 diagonals of the walked one
  bool no_front_lists = false;    // pruned sweeps: later tiers skip what an earlier one certified in place instead of running over a list of the rest
  bool no_af_split = false;       // allelicFraction by the one-launch kernel (tp / cls in LDS, every grid point screened) instead of prepare + search
  bool no_decomp_wave = false;    // decomposeAlleles by the step-wise kernel only (decompose_kernels.h) instead of the one-wave body with its working set in LDS (decompose_wave.h)
  bool no_cont16 = false;         // the band below a kept prefix row (front.h) on the tagged int32 recurrence instead of the 16-bit cells
  bool verbose = false;           // one line per pipeline stage on stderr: how many pairs took which tier (TRACYHIP_HOST_TIMERS sets it too)
  int32_t band_w = -1;            // half width of the certified band of the final alignments: -1 = from the preliminary alignment (default),
                                  // 0 = whole matrices, else [1, 4096]
  uint32_t ckpt_b = 256;
  uint32_t chain_prio = 1;        // stream-ordered orientation stage: wave priority (band16_launch.h wave_prio) of what is queued on the voted strand's side stream beside
                                  // the other strand's full sweeps.  0 = none; 1 = the tiers of the pruned sweep (place, band, certify, lists, fold) and the early
                                  // decision; 2 = also the early tail's stages (plans, scans, band launches).  Never the prefixes, the sweeps or the pass behind the decision
  uint32_t sweep_diag_period = 0; // offset form of the sweeps: steps between re-bases, clamped to what sweep_diag_period() allows; 0 = that
  uint32_t b16_multi_max = TRACY_B16_MULTI_MAX; // stream-ordered pipelines: units up to which a band stage is one launch over its four lists (launch_band16_counted)
  uint32_t front_list_min = 1024; // stream-ordered pipelines: units from which the later tiers of a pruned sweep (and the allele prefixes) run over device-side lists
  uint32_t seed_vote_cap = 2048;  // tracyhip_seed_traces: votes per trace, strand and pass held in LDS (seed.hip); more: the trace is deferred, or spills
  bool seed_spill = false;        // tracyhip_seed_traces: a trace over seed_vote_cap is answered by the spill kernel (votes counted in device memory) instead of deferred
  bool no_prefix_tall_beside = false;  // stream-ordered orientation stage, both scores exact: the voted strands' prefixes beside the other strands' full sweeps take
                                  // their shape by prefix_tall_min like every other prefix launch, instead of the tall one whatever their number
  uint32_t prefix_tall_min = 40000;  // pairs from which a launch of prefix rows alone (front.h: kFrontRows rows, one row kept) runs as eight lanes of sixteen rows
                                  // instead of sixteen of eight (launch_gotoh_ckpt_front, launch_gotoh_front_prefix_cq)
  uint32_t quad_tier_min = 32768;  // stream-ordered pipelines: units (traces, or alleles) from which the pruned sweeps get their narrow quad tier          // steps between wavefront checkpoints [32, 1024]
};
void knobs_from_env(CtxKnobs& k);
// name without the TRACYHIP_ prefix, any case; false: no such option / bad value
bool knobs_set(CtxKnobs& k, const char* name, const char* value);
std::string knobs_describe(const CtxKnobs& k);

// Reference codes (MODE_QP a2) live in ctx->dev[DB_CODES] with tracyhip::kCodePad spare bytes on both sides: the sweep kernels
// prefetch the column two steps ahead of every lane without clamping it, so idle lanes read up to 64 + 3 bytes
// before the first / behind the last base of a sequence (any byte value is a valid table row selector).
constexpr size_t kCodePad = 128;
int choose_k(uint32_t m, int mode, bool needle = false);
uint64_t seqset_extent(const tracyhip_seqset& s);

// a validated batch: descriptors in caller order + device pointers of the payloads
struct DpProblem {
  int mode = MODE_CHAR;
  bool a1_profile = false, a2_profile = false;
  const void* d_a1 = nullptr;
  const void* d_a2 = nullptr;        // MODE_QP: encoded codes
  const void* d_a2_chars = nullptr;  // the raw a2 payload on the device
  const uint8_t* d_special = nullptr;  // MODE_CQ 16-bit sweeps: block map of the a2 codes (DpArgs::special_blocks), or null
  int cq_codes = 6;                  // MODE_CQ: what the a2 columns of the batch hold -- 4: A C G T only, 5: with N, 6: anything (origin sweeps size their table by it)
  const uint8_t* d_colclass = nullptr;  // profile x profile: column classes of the a2 set (build_problem), or null
  std::vector<PairDesc> desc;
  std::vector<int> k;
};

}  // namespace tracyhip

struct tracyhip_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  uint32_t queue_prio = 0;  // CtxKnobs::chain_prio while `stream` is the voted strand's side stream beside the full sweeps (stream.hip queue_orientation), else 0:
                            // the launch helpers read it (stream.hip queued_prio)
  hipStream_t own_stream = nullptr;
  uint64_t ws_limit = 0;
  tracyhip::DevBuf dev[tracyhip::DB_COUNT];  // every device buffer the context keeps, by role (CtxDev)
  tracyhip::PinBuf pin[tracyhip::PB_COUNT];
  std::vector<tracyhip::PairDesc> cache_desc;  // descriptor / strip-height vectors of the generic DP entry points, kept between
  std::vector<int> cache_k;                    // calls (an all-pairs list is 36 MB: allocating it afresh costs 6 ms of page faults)
  std::vector<tracyhip::PairDesc> cache_full, cache_pre, cache_b16;  // the same for the orientation stage's sweep / prefix lists and the band jobs
  std::vector<tracyhip::FrontDesc> cache_fd;
  std::vector<int> cache_fullk, cache_b16k;
  tracyhip::B16Fork b16_fork;                  // side streams of the band stages (stream.hip band_stage), created with the context
  bool b16_fork_ok = false;
  bool cons_gq_ready = false;                  // CB_GQ holds the gq table of consensus.h
  hipError_t ensure_codes(size_t bytes, hipStream_t st) {
    tracyhip::DevBuf &d_codes = dev[tracyhip::DB_CODES], &d_special = dev[tracyhip::DB_SPECIAL];
    hipError_t e = d_codes.ensure(bytes + 2 * tracyhip::kCodePad);
    if (e != hipSuccess) return e;
    // pads hold code 0 ('A'): an ordinary column for every kernel
    if ((e = hipMemsetAsync(d_codes.p, 0, tracyhip::kCodePad, st)) != hipSuccess) return e;
    if ((e = hipMemsetAsync(static_cast<uint8_t*>(d_codes.p) + tracyhip::kCodePad + bytes, 0, tracyhip::kCodePad, st)) != hipSuccess) return e;
    // one byte per 256 code bytes: set by the encoders where a block holds an N or '-' / other code (DpArgs::special_blocks)
    if ((e = d_special.ensure((bytes >> 8) + 2)) != hipSuccess) return e;
    return hipMemsetAsync(d_special.p, 0, (bytes >> 8) + 2, st);
  }
  uint8_t* special_blocks() const { return static_cast<uint8_t*>(dev[tracyhip::DB_SPECIAL].p); }
  uint8_t* codes() const { return static_cast<uint8_t*>(dev[tracyhip::DB_CODES].p) + tracyhip::kCodePad; }
  bool aftab_ready = false;
  uint64_t ws_cache_budget = 0, ws_cache_held = 0;  // stream.hip workspace_budget: the last answer and what the context held then
  uint32_t ws_cache_share = 0;
  bool declut_ready = false;
  uint32_t b16_round = 0;
  // kernel timing
  struct Pending { int which; hipEvent_t e0, e1; uint64_t cells, bytes; };
  // lanes: further contexts (own stream, own buffers) the batch pipelines split a call over, one host thread each
  // (tracyhip_set_lanes); this context is the first lane, empty = the pipelines run on it alone
  std::vector<tracyhip_ctx*> lanes;
  uint32_t mem_share = 1;  // contexts planning workspace on this device at the same time (lanes of one call): each takes its share of what is free
  bool timing = false;
  tracyhip::CtxKnobs knobs;  // (the fields below it used to be: no_narrow, no_compact, no_screen)
  tracyhip_call_stats stats = {};  // tiers of the last pipeline call (tracyhip_last_call_stats)
  tracyhip_pad_stats pad_stats = {};  // of the last tracyhip_pad_traces call (tracyhip_last_pad_stats)
  tracyhip_render_stats render_stats = {};  // of the last tracyhip_render_traces call (tracyhip_last_render_stats)
  tracyhip_read_stats read_stats = {};  // of the last tracyhip_read_traces call (tracyhip_last_read_stats)
  tracyhip_alntext_stats alntext_stats = {};  // of the last tracyhip_render_alignments call (tracyhip_last_alntext_stats)
  tracyhip_dcptext_stats dcptext_stats = {};  // of the last tracyhip_render_decompositions call (tracyhip_last_dcptext_stats)
  std::vector<Pending> pending;
  std::vector<hipEvent_t> free_events;
  tracyhip_kernel_timing acc[TRACYHIP_TIMER_COUNT] = {};
  // asynchronous calls (tracyhip_*_async): executed in issue order by one worker thread per context
  struct AsyncState {
    std::mutex m;
    std::condition_variable cv;
    std::deque<std::function<int()>> q;
    std::thread worker;
    std::thread::id worker_id;
    bool busy = false, stop = false;
    int rc = TRACYHIP_OK;      // first error since the last synchronize
    std::string msg;
  };
  AsyncState* async = nullptr;
  void release_all() {
    for (auto& b : dev) b.release();
    for (auto& b : pin) b.release();
    aftab_ready = declut_ready = cons_gq_ready = false;  // what the freed buffers held
  }
};

namespace tracyhip {
// The per-trace host loops of the pipelines (descriptors, bands, verdicts of 10^5 traces between two launches) on a few threads:
// fn(lo, hi, tid) over [0, n) in contiguous slices; small n runs inline.
constexpr uint32_t kHostThreads = 8;
static_assert(kHostThreads <= kPlanSlices, "the plans of dp_plan.h keep one partial sum per slice");
// Workers that stay alive between calls (starting seven threads costs ~0.3 ms, and a decompose call of 10^5 traces runs forty of
// these loops between its launches).  One job at a time: a second caller (another lane) gets `false` and starts its own threads.
bool host_pool_run(const std::function<void(uint32_t)>& job);  // job(slice) for slice = 0 .. kHostThreads - 1, worked off by the pool + the caller
uint32_t host_pool_threads();  // threads a job runs on: TRACYHIP_HOST_THREADS, or the cores the process may use, at most kHostThreads
template <class Fn>
void parallel_for(uint32_t n, Fn fn) {
  if (n < 16384u) { fn(0u, n, 0u); return; }
  auto lo = [&](uint32_t t) { return (uint32_t)((uint64_t)n * t / kHostThreads); };
  if (host_pool_run([&](uint32_t t) { fn(lo(t), lo(t + 1), t); })) return;
  // the pool is busy with another lane's loop: threads of our own, no more than the process's share
  std::atomic<uint32_t> next(0);
  auto work = [&]() { for (uint32_t t = next.fetch_add(1); t < kHostThreads; t = next.fetch_add(1)) fn(lo(t), lo(t + 1), t); };
  std::vector<std::thread> th;
  const uint32_t nth = host_pool_threads();
  th.reserve(nth);
  for (uint32_t t = 1; t < nth; ++t) th.emplace_back(work);
  work();
  for (auto& x : th) x.join();
}
// A DpProblem borrows the context's descriptor vectors for its lifetime and hands them back, whatever the way out: batches of
// 10^5 pairs are megabytes of descriptors per stage, and allocating them afresh costs a millisecond of page faults each time.
// (One lease at a time per context: the stages of a pipeline build their problems one after the other.)
struct DpProblemLease {
  tracyhip_ctx* c;
  DpProblem& p;
  DpProblemLease(tracyhip_ctx* c_, DpProblem& p_) : c(c_), p(p_) {
    p.desc.swap(c->cache_desc); p.k.swap(c->cache_k);
    p.desc.clear(); p.k.clear();
  }
  ~DpProblemLease() { p.desc.swap(c->cache_desc); p.k.swap(c->cache_k); }
  DpProblemLease(const DpProblemLease&) = delete;
  DpProblemLease& operator=(const DpProblemLease&) = delete;
};
// the same for a band job (Band16Job, below): entries whose strip height is 0 are never read, so stale descriptors may stay in them
template <class Job>
struct Band16Lease {
  tracyhip_ctx* c;
  Job& j;
  Band16Lease(tracyhip_ctx* c_, Job& j_) : c(c_), j(j_) { j.desc.swap(c->cache_b16); j.k.swap(c->cache_b16k); }
  ~Band16Lease() { j.desc.swap(c->cache_b16); j.k.swap(c->cache_b16k); }
  Band16Lease(const Band16Lease&) = delete;
  Band16Lease& operator=(const Band16Lease&) = delete;
};
// Host-side profile of the pipelines (TRACYHIP_HOST_TIMERS=1): wall time of the labelled scopes, summed per label and printed to
// stderr when the process ends.  For finding where the host keeps the GPU waiting between two launches; off = one branch.
struct HostScope {
  const char* label;
  uint64_t t0;
  explicit HostScope(const char* l);
  ~HostScope();
};
#define TRACYHIP_HOST_SCOPE(name, label) tracyhip::HostScope name(label)
int timing_begin(tracyhip_ctx* ctx, int which, uint64_t cells, uint64_t bytes);  // record start event
int timing_end(tracyhip_ctx* ctx);                                              // record stop event
int timing_collect(tracyhip_ctx* ctx);                                          // after a stream sync
int ctx_begin(tracyhip_ctx* ctx);
// hipStreamSynchronize(ctx->stream), counted in tracyhip_call_stats::host_syncs
inline hipError_t ctx_sync(tracyhip_ctx* ctx) { ctx->stats.host_syncs += 1; return hipStreamSynchronize(ctx->stream); }
// what a RunMerger (ragged_plan.h) does with a finished run on the device side: array k's bytes from its part of a staging buffer
// into the caller's array, queued on the context's stream
template <int N>
struct CopyBackRun {
  tracyhip_ctx* ctx;
  const uint8_t* src[N];
  uint8_t* dst[N];
  hipError_t operator()(int k, uint64_t s, uint64_t d, uint64_t bytes) const {
    return hipMemcpyAsync(dst[k] + d, src[k] + s, bytes, hipMemcpyDeviceToHost, ctx->stream);
  }
};
int async_submit(tracyhip_ctx* ctx, std::function<int()> fn);  // queue a call on the context's worker thread
int async_drain(tracyhip_ctx* ctx);                           // wait for the queue; returns (and clears) the first error
// the _async twin of a batch call fn(ctx, job, mem, out): job and result structs are copied now (the arrays they point to stay the
// caller's until the queue has drained), the call is queued
template <class Job, class Res>
int async_twin(int (*fn)(tracyhip_ctx*, const Job*, int, const Res*), tracyhip_ctx* ctx, const Job* job, int mem, const Res* out) {
  if (!ctx || !job || !out) return set_error(TRACYHIP_ERR_ARG, "null context / job / result");
  const Job j = *job;
  const Res o = *out;
  return async_submit(ctx, [=]() { return fn(ctx, &j, mem, &o); });
}
// a tracyhip_last_*_stats getter over the counters a call keeps in its context
template <class Stats>
int last_stats(tracyhip_ctx* ctx, Stats tracyhip_ctx::*stats, Stats* out) {
  if (!ctx || !out) return set_error(TRACYHIP_ERR_ARG, "null context / out");
  *out = ctx->*stats;
  return TRACYHIP_OK;
}
// Staging of a caller's array.  MEM_DEVICE: it is used in place.  MEM_HOST: it goes through a grow-only buffer of the context.
// stage_in: a read-only input, uploaded (zero bytes: the caller's pointer, nothing allocated).
// stage_out: a result array, optionally uploaded first (zero bytes: one byte allocated, so the pointer is a device pointer);
// unstage copies it back after the launches.  Nothing here waits for the stream.
int stage_in(tracyhip_ctx* ctx, DevBuf& buf, const void* src, uint64_t bytes, int mem, const void** dev);
int stage_out(tracyhip_ctx* ctx, DevBuf& buf, void* user, uint64_t bytes, int mem, bool upload, void** dev);
int unstage(tracyhip_ctx* ctx, void* user, const void* dev, uint64_t bytes, int mem);
int check_params(const tracyhip_params* prm, uint64_t max_mn);
// The workspace a context may plan with: the caller's limit (tracyhip_set_workspace_limit), else this context's share of 70 % of what
// is free on the device now plus `held`, the bytes it already holds for the purpose.  (A driver call: each site has its own
// precondition for asking at all.)
int workspace_limit(tracyhip_ctx* ctx, uint64_t held, uint64_t* limit);
// ... with the driver's answer kept for as long as the context holds what it held when it asked (stream.hip; from_cache: the answer
// was a kept one)
int workspace_budget(tracyhip_ctx* ctx, uint64_t held, uint64_t* out, bool* from_cache = nullptr);
// a seqset of profiles as the batch calls take one: its kind and arrays; then that the profiles [lo, hi) have columns.  false: the
// error is set (`name` opens the message)
bool check_profile_set(const tracyhip_seqset& s, const char* name);
bool check_profile_columns(const tracyhip_seqset& s, const char* name, uint32_t lo, uint32_t hi);
// (the stages of run_dp -- DP_PLAIN, DP_CKPT, DP_BAND, DP_PREFIX, DP_ORIGIN -- are dp_plan.h's)
struct DpCkpt {
  int32_t* d_ckpt = nullptr;
  int32_t* d_lastrow = nullptr;
  uint32_t B = 256;
  bool narrow = false;  // set by the DP_CKPT stage (16-bit kernel used), read by the DP_BAND stage
  uint32_t* d_ends = nullptr;  // DP_ORIGIN: two entries per pair, indexed by PairDesc::out
  const uint32_t* d_votes = nullptr;  // DP_CKPT of both orientations: orientation votes (DpArgs::votes), or null
  uint32_t vote_nt = 0;
};
// origin-tracking sweep: one pass of strip height K, columns and scores inside the packed fields (dp_lane.h origin_step)
bool origin_ok(const tracyhip_params* prm, uint32_t maxm, uint32_t maxn, int K);
int run_ckpt_prefix(tracyhip_ctx* ctx, const void* d_a1, const void* d_a2, const std::vector<PairDesc>& full, const std::vector<int>& fullk,
                    const std::vector<PairDesc>& pre, const tracyhip_params* prm, int32_t* d_scores, DpCkpt* ck, bool front_shape = false);
// defer_herr (kErrWords host words that live until the caller has waited for the stream; traceback of strings only): the launches are
// queued and the error words copied there WITHOUT a wait -- the caller synchronises behind its own launches and passes the words to
// range_verdict itself (no narrow launches; max_mn, kTagShift).  The pinned descriptors are the context's: no second run_dp before that wait.
int run_dp(tracyhip_ctx* ctx, const DpProblem& pb, const tracyhip_params* prm, bool needle, bool trace,
           int32_t* d_scores, uint8_t* d_ops, const uint64_t* d_ops_off, uint32_t* d_ops_len, int stage = DP_PLAIN,
           DpCkpt* ck = nullptr, int32_t* defer_herr = nullptr);
bool narrow_ok(const tracyhip_params* prm, uint32_t maxm, int K, int64_t Q = 0);
// the offset form of the 16-bit query-profile sweeps: steps between re-bases for strips of K rows on `lanes` lanes per pair, 0 = no room
uint32_t sweep_diag_period(const tracyhip_params* prm, int K, int lanes, int64_t Q = 0);
// ... for a launch of this context (options no_sweep_diag / sweep_diag_period; 0: the launch takes the form without offsets)
uint32_t ctx_sweep_diag(const tracyhip_ctx* ctx, const tracyhip_params* prm, int K, int lanes);
// ... for a launch of full sweeps and prefix groups, which takes one form: sets both periods or neither, and counts the launch in the statistics
void launch_diag_periods(tracyhip_ctx* ctx, const tracyhip_params* prm, int K, uint32_t nfull, uint32_t npre, bool front_shape, tracyhip::DpArgs& full, tracyhip::DpArgs& pre);
// entry of a narrow_launches list for a sweep that ran in the offset form: range_verdict re-evaluates the period with the Q it finds
inline int narrow_launch_diag(int K, uint32_t period) { return K | (int)(period << 8); }
// profile x profile score kernel with 16-bit cells for pairs of at most max_mn = m + n (Q: largest substitution score, 0 = a priori)
bool arith16_ok(const tracyhip_params* prm, uint64_t max_mn, int64_t Q);
int32_t sub_limit(const tracyhip_params* prm);
// sweep arguments with what a tracyhip_params decides: the scoring fields, qlimit and the context's error words
DpArgs scoring_args(tracyhip_ctx* ctx, const tracyhip_params* prm);
// largest |match| / |mismatch| whose table entries x 32 (tagged tracebacks, band kernels) fit int16; wider scorings take slower forms
constexpr int32_t kWideScore = 1000;
// device error block (DpArgs::err): kErrWords words owned by the DP launches + one verdict word of the pipelines' reference check
constexpr int kErrVerdictWord = kErrWords;
constexpr int kErrSweptWord = kErrWords + 2;  // 64-bit counter of the band traceback (DpArgs::swept), 8-byte aligned
constexpr size_t kErrBytes = sizeof(int32_t) * (kErrWords + 4);
// internal status (never returned through the C ABI): a 16-bit launch ran outside its proven value range; repeat on int32
constexpr int kWiden = 1;
int range_verdict(const tracyhip_params* prm, const int32_t* herr, const std::vector<std::pair<uint32_t, int>>& narrow_launches,
                  uint64_t max_mn, int value_shift);
int build_problem(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, int mem, bool needle, DpProblem& pb, uint64_t* max_mn);

// ---- profile batches (prof_batch.hip): what build_problem, consensus_run and assemble_run share ----
struct ProfSeq {  // one profile of a batch: float offset and columns
  uint64_t off;
  uint32_t len, pad;
};
// revcomp of n profiles (profile.h:74-90): profile s is read at in + off and written at out + rev_base + off
hipError_t launch_prof_revcomp(const ProfSeq* seqs, uint32_t n, const float* in, float* out, uint64_t rev_base, hipStream_t st);
// zero[s] = row 4 ('N') of profile s is all zero (chooses the 16-term score body); colclass (or null) receives the class of every
// column, indexed like row 0 of `data`
hipError_t launch_prof_classify(const ProfSeq* seqs, uint32_t n, const float* data, uint8_t* zero, uint8_t* colclass, hipStream_t st);
// The launch loop of the batch calls over units [lo, hi) of a sorted descriptor list (hd: host copy, dd: device copy, k[u]: strip
// height of unit u): one launch per run of equal strip height and PAIR_ROW4_ZERO.  `args` carries everything but the pairs and the
// walk pointers.
// score form, two descriptors per unit (both strands): 16-bit cells where !wide, !no_narrow and arith16_ok hold for the run's largest
// m + n, which is then appended to narrow_launches for range_verdict; timed as TRACYHIP_TIMER_SCORE
// (per: descriptors per unit -- 1 where the caller's profiles are already oriented and only one strand is scored)
int prof_score_runs(tracyhip_ctx* ctx, const tracyhip_params* prm, bool wide, const DpArgs& args, const PairDesc* hd, const PairDesc* dd,
                    const int* k, uint32_t lo, uint32_t hi, std::vector<std::pair<uint32_t, int>>& narrow_launches, uint32_t per = 2);
// traceback form, one descriptor per unit: the sweep walks its pairs itself (ops / ops_off / ops_len by PairDesc::out), or with
// no_fused_walk a walk launch follows each sweep; timed as TRACYHIP_TIMER_TRACE / TRACYHIP_TIMER_WALK
int prof_trace_runs(tracyhip_ctx* ctx, const DpArgs& args, const PairDesc* hd, const PairDesc* dd, const int* k, uint32_t lo, uint32_t hi,
                    uint8_t* ops, const uint64_t* ops_off, uint32_t* ops_len);

// ---- row blocks of `tracy assemble` (msa_batch.hip over assemble_wave.h): what assemble_run and denovo_run share ----
struct AsmStep {       // one merge: a chain step of a group (assemble.hip) or a tree node (denovo.hip)
  MsaSide left, right; // the rows above / below in the merged block: an input profile (rows == null) or a block of rows
  uint64_t ops_off;    // the merge's op string in the ops buffer
  uint32_t slot;       // its entry of ops_len (PairDesc::out)
  uint32_t cap;        // left.c + right.c: more ops than that cannot be (nothing is written otherwise)
  uint8_t* dst;        // (left.n + right.n) rows x ops_len columns
  int32_t* span;       // 2 per row of dst
  float* prof;         // msa_profile of dst, 6 x ops_len -- or null: nothing aligns against this block
  uint8_t* colclass;   // classes of its columns
};
struct AsmFinal {      // one finished group
  const uint8_t* rows;
  const int32_t* span;
  uint32_t rows_used;  // the rows consensus() looks at
  uint32_t slot;
  int32_t cov_threshold;
  uint32_t cap;
  uint8_t *gapped, *cons, *qual;
  uint32_t* cons_len;
};
// steps / fin: device arrays of n entries; ops_len is indexed by their slots.  One wave per (step, row of the merged block) with
// max_rows the largest left.n + right.n; one wave per (step, 64 columns) with max_cap the largest cap; one wave per finished group.
hipError_t launch_msa_merge(const AsmStep* steps, uint32_t n, uint32_t max_rows, const uint8_t* ops, const uint32_t* ops_len, hipStream_t st);
hipError_t launch_msa_profile(const AsmStep* steps, uint32_t n, uint64_t max_cap, const uint32_t* ops_len, hipStream_t st);
hipError_t launch_msa_consensus(const AsmFinal* fin, uint32_t n, const uint32_t* ops_len, hipStream_t st);

// ---- group batches (msa_batch.hip): the host code around those kernels that assemble_run and denovo_run share ----
// The result fields tracyhip_assemble_result and tracyhip_denovo_result have in common, and where the kernels write the payload
// arrays: the caller's own (MEM_DEVICE) or one staging buffer in the caller's layout (MEM_HOST: AB_PAY, which DN_PAY aliases).
struct GroupOut {
  uint32_t ng;
  uint32_t *nrows, *ncol, *cons_len;
  uint8_t *rows, *gapped, *cons, *qual;
  const uint64_t *rows_offset, *col_offset;
  uint8_t *d_rows = nullptr, *d_gapped = nullptr, *d_cons = nullptr, *d_qual = nullptr;  // set by bind()
  uint32_t* d_clen = nullptr;
  template <class Result>
  GroupOut(uint32_t ng_, const Result& r)
      : ng(ng_), nrows(r.nrows), ncol(r.ncol), cons_len(r.cons_len), rows(r.rows), gapped(r.gapped), cons(r.cons), qual(r.qual),
        rows_offset(r.rows_offset), col_offset(r.col_offset) {}
  // a call whose groups hold no trace: nrows, ncol and cons_len are 0 everywhere (MEM_DEVICE: one synchronisation)
  int clear_counts(tracyhip_ctx* ctx, int mem) const;
  // the payload pointers; ext_rows / ext_col: the largest offset + capacity over the groups that hold a trace.  d_clen is cleared
  int bind(tracyhip_ctx* ctx, int mem, uint64_t ext_rows, uint64_t ext_col);
  // the entry of a finished group for msa_consensus: its rows are the first rows_used of the block at rows_offset[g]
  AsmFinal final_entry(uint32_t g, const int32_t* span, uint32_t rows_used, uint32_t slot, uint32_t cap, float fraction_called) const;
  // queued behind the last launch: nrows / ncol from the host's h_nrows / h_ncol, and for a host caller cons_len and what every group
  // wrote of rows / gapped / cons / qual.  The caller synchronises
  int copy_back(tracyhip_ctx* ctx, int mem, const uint32_t* h_nrows, const uint32_t* h_ncol) const;
};
// `bytes` of a result array the host computed, into the caller's array: copied (MEM_HOST) or queued as an upload (MEM_DEVICE)
int put_result(tracyhip_ctx* ctx, int mem, void* user, const void* host, size_t bytes);
// One batch of traceback sweeps through prof_trace_runs: the descriptors in launch order (the caller sorts by strip height and row-4
// flag), where each sweep's planes and boundary rows start, and the op strings the walks write (indexed by PairDesc::out).
struct TraceBatch {
  PairDesc *hd = nullptr, *dd = nullptr;  // PB_DESC / DB_DESC, sized by the caller
  uint8_t* ops = nullptr;                 // the op strings: string PairDesc::out at ops + ops_off[out], ops_len[out] bytes
  const uint64_t* ops_off = nullptr;
  uint32_t* ops_len = nullptr;
  uint64_t limit = 0;                     // workspace_limit: what the planes and boundary rows of one batch may take
  std::vector<int> k;                     // strip heights, in launch order
  uint64_t words = 0, scr = 0;            // running sums: traceback words, boundary-row pairs
  void clear() { k.clear(); words = scr = 0; }
  // gotoh(a1, a2): m rows at float offset a1_off of DpArgs::a1 against n columns at a2_off of DpArgs::a2, strips of K rows
  void add(uint64_t a1_off, uint32_t m, uint64_t a2_off, uint32_t n, bool row4_zero, int K, uint32_t out);
  // DB_BITS / DB_SCRATCH hold the batch (grown if need be, refused above the limit) and are bound to `a`; the descriptors are uploaded
  int upload(tracyhip_ctx* ctx, DpArgs& a) const;
};
// the descriptor of one profile x profile pair (bits_off / scratch_off / out are the caller's)
PairDesc prof_pair_desc(uint64_t a1_off, uint32_t m, uint64_t a2_off, uint32_t n, bool row4_zero);
// One batch of merges: the sweeps of `tb` (entry j is the pair of h_step[j]: left x right), msa_merge, msa_profile where a step has a
// profile, then ops_len[lo, hi) read back into h_len[lo, hi) and ONE synchronisation.  The caller checks h_len against the caps.
int msa_merge_batch(tracyhip_ctx* ctx, DpArgs& a, const TraceBatch& tb, const AsmStep* h_step, AsmStep* d_step, uint32_t* h_len, uint32_t lo,
                    uint32_t hi);
// msa_consensus of the nf finished groups of a chunk (h_fin: pinned, filled through GroupOut::final_entry); nothing is waited for
int msa_consensus_batch(tracyhip_ctx* ctx, const AsmFinal* h_fin, AsmFinal* d_fin, uint32_t nf, const uint32_t* ops_len);
// The tail of the strand-score stage over nu sorted units (two descriptors each, uploaded by the caller; `a` carries the payload
// pointers): DB_ERR cleared, prof_score_runs, the nscores scores of a.scores and the error words read back, one synchronisation,
// range_verdict -- kWiden: a 16-bit launch met an un-normalised profile, the caller repeats on int32
int prof_score_stage(tracyhip_ctx* ctx, const tracyhip_params* prm, bool wide, DpArgs& a, const PairDesc* hd, const PairDesc* dd, const int* k,
                     uint32_t nu, int32_t* h_scores, size_t nscores, uint64_t max_mn, std::vector<std::pair<uint32_t, int>>& narrow_launches);

// ---- band kernels (band16.h): Gotoh on a diagonal band, four pairs per wave ----
// a batch for them: descriptors whose a1_off / a1_stride point into the substitution tables d_qp (build_b16_tables), a2_off into
// d_codes (codes 0..5), ckpt_off = band_pack(dmin, dmax); k[i] = strip height of pair i (b16_pick_k)
struct Band16Job {
  int kind = 0;                 // 0: traceback words + walk (scores, ops); 1: origin-tracking sweep (scores, ends)
  const int16_t* d_qp = nullptr;
  const uint8_t* d_codes = nullptr;
  std::vector<PairDesc> desc;
  std::vector<int> k;           // 4 / 8 / 12; 0: the pair is not part of the job (callers fill both vectors for every trace, in order)
};
// substitution tables of `desc.size()` sequences (b16_table_kernel): entries are scores << kTagShift; desc[i].out_off / stride are
// filled in here, the buffer is (re)sized.  strings: a1 holds bytes, else float profiles.
int build_b16_tables(tracyhip_ctx* ctx, DevBuf& buf, const void* d_a1, bool strings, std::vector<B16TableDesc>& desc, const tracyhip_params* prm);
int run_band16(tracyhip_ctx* ctx, Band16Job& job, const tracyhip_params* prm, int32_t* d_scores, uint32_t* d_ends, uint8_t* d_ops,
               const uint64_t* d_ops_off, uint32_t* d_ops_len);
// The pruned orientation sweep (front.h) of fd.size() pairs whose prefix rows are in d_row (PAIR_KEEP_ROW): band placed, band swept
// below the kept row (strip height K, band of 2 halfw + 1 diagonals), certificate.  FrontDesc::out must be the pair's index in fd.
// Host results per pair: fo (ok: the score is gotohScore), score, c_e as a window column (0: none).
struct FrontResult {
  std::vector<FrontOut> fo;
  std::vector<int32_t> score;
  std::vector<uint32_t> ce;
};
// d_codes: the codes the band kernels read (null: the context's); keep_err: the error words hold the flags of a launch that has
// not been read yet (run_prefix_keep_cq) -- they are not cleared, and reported with this call's
int run_front(tracyhip_ctx* ctx, const std::vector<FrontDesc>& fd, const int16_t* d_qp, const uint32_t* d_row, const tracyhip_params* prm,
              FrontResult& out, const uint8_t* d_codes = nullptr, bool keep_err = false);
// The prefix rows of the pruned sweep for string x code pairs (gotoh(allele, window), indigo.h:359): rows 1 .. kFrontRows of every
// pair over all its columns, row kFrontRows kept at d_lastrow + PairDesc::lastrow_off (PAIR_KEEP_ROW).  Queued, not waited for: the
// error words are cleared before the launch and read by the run_front call that follows.
int run_prefix_keep_cq(tracyhip_ctx* ctx, const void* d_a1, const void* d_a2, const uint8_t* d_special, const std::vector<PairDesc>& pre,
                       const tracyhip_params* prm, int32_t* d_lastrow);
}  // namespace tracyhip
#endif
