/*
 * tracy_hip.h -- C ABI of the MI355X-native tracy alignment / deconvolution hot path.
 *
 * The reference (gear-genomics/tracy v0.9.1) has no FFI: its boundary for this path is the set of
 * header-only C++ templates listed below.  Each entry point here is the batched, device-side
 * replacement for one of them; tracy_amd/host/tracy_amd.hpp keeps the reference's per-call C++
 * signatures (batch of one) on top of this ABI, INTEGRATION.md shows the binding a tracy maintainer
 * would add.
 *
 *   reference interface (under /root/reference/src)                         replaced by
 *   -------------------------------------------------------------------     ---------------------------
 *   gotohScore(a1,a2,ac,sc)                gotoh.h:12-68                    tracyhip_gotoh_score
 *   gotoh(a1,a2,align,ac,sc)               gotoh.h:71-174                   tracyhip_gotoh_align
 *   needleScore / needle                   needle.h:12-57 / 59-138          tracyhip_needle_score / _align
 *   _createAlignment (string / profile)    align.h:196-223, 254-293         tracyhip_alignment_rows
 *   DnaScore<int>, AlignConfig<H,V>        align.h:11-32, 37-80             tracyhip_params
 *   sage() hot section                     sage.h:191-311                   tracyhip_align_traces
 *   indigo() hot section                   indigo.h:190-388                 tracyhip_decompose_traces
 *   findBreakpoint                         decompose.h:7-56                 tracyhip_find_breakpoint
 *   findHomozygousBreakpoint               decompose.h:59-128               tracyhip_find_homozygous_breakpoint
 *   decomposeAlleles                       decompose.h:179-376              tracyhip_decompose_alleles
 *   generateSecondaryDecomposed            decompose.h:378-410              tracyhip_secondary_decomposed
 *   allelicFraction                        decompose.h:412-621              tracyhip_allelic_fraction
 *   trimReferenceSlice                     fmindex.h:429-463                tracyhip_trim_reference_slice
 *   callVariants / insertVariant           variants.h:34-126                tracyhip_call_variants
 *   indigo() variant section               indigo.h:397-423, 442-443        tracyhip_decompose_variants
 *   getReferenceSlice (indexed genome)     fmindex.h:236-326                tracyhip_seed_traces
 *   consensus() hot section                consensus.h:501-577              tracyhip_consensus_traces
 *   basecall + estimateQualities           abif.h:408-511, 164-253          tracyhip_basecall_traces
 *     trimTrace / createProfile(tr, bc)    trim.h:35-73 / profile.h:21-52   (same call)
 *     gtLetter / pairwiseConsensus         consensus.h:94-171 / 189-238     (consensus_kernel, same call)
 *   assemble(), reference-guided chain     assemble.h:219-288               tracyhip_assemble_traces
 *   assemble(), de novo                    assemble.h:378-471, msa.h:33-368 tracyhip_denovo_traces
 *     _createProfile(char MSA) / consensus align.h:138-180 / msa.h:165-254   (msa_profile / msa_consensus kernels, same call)
 *
 * Conventions
 *   - plain C types only; the caller owns every buffer passed in; nothing is retained after return.
 *   - "metadata on the host, payload where `mem` says": offset / length / index arrays are ALWAYS host
 *     arrays; sequence payloads and result arrays are host pointers (TRACYHIP_MEM_HOST, staged through
 *     the library's device buffers) or device pointers (TRACYHIP_MEM_DEVICE, zero copy).
 *   - every call returns TRACYHIP_OK (0) or a negative error; tracyhip_last_error() gives the text.
 *     The reference's DP functions cannot fail (gotoh.h has no checks); the extra errors here are
 *     bad arguments, HIP failures, out-of-memory and parameter ranges the int32 kernels cannot hold.
 *   - there is NO CPU fallback: without a usable gfx950 device every compute call fails.
 */
#ifndef TRACY_HIP_H
#define TRACY_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TRACYHIP_OK 0
#define TRACYHIP_ERR_ARG (-1)      /* NULL pointer, inconsistent sizes */
#define TRACYHIP_ERR_HIP (-2)      /* a HIP runtime call failed */
#define TRACYHIP_ERR_OOM (-3)      /* device or host allocation failed */
#define TRACYHIP_ERR_RANGE (-4)    /* scores / lengths outside what the int32 kernels represent */
#define TRACYHIP_ERR_NODEVICE (-5) /* no gfx950 device visible */

#define TRACYHIP_MEM_HOST 0
#define TRACYHIP_MEM_DEVICE 1

/* sequence payload kinds: what TAlign1/TAlign2 is in the reference call */
#define TRACYHIP_SEQ_CHAR 0    /* std::string: raw bytes, scored by byte equality (align.h:96-101) */
#define TRACYHIP_SEQ_PROFILE 1 /* boost::multi_array<float,2>[6][len], p[k][j] at k*len+j (align.h:103-118) */

typedef struct tracyhip_ctx tracyhip_ctx;

/* DnaScore<int> (align.h:11-32; inf is the fixed 1000000) + AlignConfig<hfree,vfree> (align.h:37-80).
 * |match|, |mismatch| <= 30000 and (m + n) * (|go| + |ge| + max(|match|, |mismatch|)) + 10^6 < 2^26 (TRACYHIP_ERR_RANGE beyond: the
 * exact range of the x 32 tagged int32 tracebacks); beyond |1000| the table-driven and banded forms give way to slower exact ones */
typedef struct {
  int32_t match;
  int32_t mismatch;
  int32_t go;
  int32_t ge;
  int32_t hfree; /* THorizontal: horizontal moves are free on the first and last ROW */
  int32_t vfree; /* TVertical:   vertical moves are free on the first and last COLUMN */
} tracyhip_params;

/* a set of sequences packed back to back */
typedef struct {
  int32_t kind;           /* TRACYHIP_SEQ_* */
  const void* data;       /* chars, or floats: sequence s occupies [offset[s], offset[s] + (kind ? 6 : 1) * length[s]) */
  const uint64_t* offset; /* HOST array, element offsets (bytes for CHAR, floats for PROFILE) */
  const uint32_t* length; /* HOST array, number of columns */
  uint32_t count;         /* number of sequences */
} tracyhip_seqset;

/* npairs independent DP problems: pair i aligns a1[a1_index[i]] (rows) with a2[a2_index[i]] (columns) */
typedef struct {
  uint32_t npairs;
  tracyhip_seqset a1;
  tracyhip_seqset a2;
  const uint32_t* a1_index; /* HOST array or NULL (= identity) */
  const uint32_t* a2_index; /* HOST array or NULL (= identity) */
} tracyhip_pairs;

/* ---- lifecycle --------------------------------------------------------------------------------- */
/* Host threads: the per-trace loops the pipelines run between two launches (descriptors, bands, verdicts) use a few worker
   threads of the process -- as many as it may run on, at most 8; TRACYHIP_HOST_THREADS=<n> in the environment sets the number
   (one process per GPU on a shared node: the cores of the node divided by the local ranks). */
int tracyhip_device_count(int* count);
int tracyhip_create(int device, tracyhip_ctx** ctx);
int tracyhip_destroy(tracyhip_ctx* ctx);
/* run on a caller-owned hipStream_t (e.g. torch.cuda.current_stream().cuda_stream); NULL = own stream */
int tracyhip_set_stream(tracyhip_ctx* ctx, void* hip_stream);
/* upper bound for the library's device workspace (traceback planes are chunked to fit); 0 = default */
int tracyhip_set_workspace_limit(tracyhip_ctx* ctx, uint64_t bytes);
/* Lanes (1..8, default 1): tracyhip_align_traces / tracyhip_decompose_traces split a batch into `lanes` contiguous
   chunks and run them concurrently, each on its own stream with its own workspace and host thread.  The chunks'
   kernels fill each other's tails and the host stages between kernels (orientation decision, trimReferenceSlice
   geometry) overlap with device work; results are the same arrays as with one lane.  The calls stay synchronous:
   inputs enqueued on the context's stream are waited for, everything is complete on return.  Needs the per-trace
   result regions (ops_offset) in trace order; otherwise the call runs on one lane. */
int tracyhip_set_lanes(tracyhip_ctx* ctx, uint32_t lanes);
/* waits for the context's stream AND for every *_async call issued on the context; returns the first error one of those
   calls produced since the last synchronize (tracyhip_last_error() then holds its text), TRACYHIP_OK otherwise */
int tracyhip_synchronize(tracyhip_ctx* ctx);
/* Options.  Every switch of the library is read from the environment ONCE, when a context is created (TRACYHIP_<NAME>, e.g.
   TRACYHIP_NO_STREAM=1), and changed afterwards only through this call; name is the variable without the prefix, in any case:
     no_stream (pipelines planned by the host between launches instead of stream-ordered), no_narrow, no_compact, no_screen,
     no_band, no_band16, no_front, no_prefix, no_vote, no_origin, no_subwindow, no_prelim_origin, no_cq, no_fused_walk, no_cont16, no_quads, no_fork, no_early_tail (`tracy align`: no alignment queued before both orientation scores are known), no_decomp_wave, no_af_split, no_front_lists, no_origin_band, sweeps_alone (measurement: the full sweeps of the orientation stage on a device of their own), no_sweep_diag (16-bit sweeps on values as they are instead of the diagonal-offset form), no_prefix_tall_beside (see prefix_tall_min)   "0" / "1"
     sweep_diag_period  (steps between re-bases of the offset form: 0 = what the range rule allows, else a multiple of 4 from 64 on, clamped to that)
     band_w  (half width of the certified band of the final alignments; -1 = from the preliminary alignment, 0 = whole matrices)
     ckpt_b  (steps between wavefront checkpoints, 32 .. 1024)      verbose  (one line per pipeline stage on stderr)
     seed_vote_cap  (tracyhip_seed_traces: votes one trace may collect per strand and pass on the device, 1 .. 2048, default 2048;
                    a trace with more is DEFERRED to host seeding -- the caller's results stay the same -- or, with seed_spill, spills)
     seed_spill     ("0" / "1", default "0": a trace over seed_vote_cap is answered on the device by the spill launch of tracyhip_seed_traces,
                    its votes counted in device memory, instead of DEFERRED; any other value is refused)
     quad_tier_min  (stream-ordered pipelines: traces / alleles from which a pruned sweep gets its narrow first tier; default 32768)
     prefix_tall_min (pairs from which a launch of the pruned sweeps' prefix rows alone runs as eight lanes of sixteen rows instead of sixteen
                    of eight; 0 .. 2147483647, default 40000.  The voted strands' prefixes that the stream-ordered orientation stage queues beside
                    the other strands' full sweeps take the sixteen-row shape whatever their number, unless no_prefix_tall_beside is "1")
     front_list_min (... from which its later tiers, and the allele prefixes of `tracy decompose`, run over device-side lists of the units
                    that are left instead of skipping the others in place; default 1024)
     b16_multi_max  (stream-ordered pipelines: units up to which a band stage is ONE launch over its four lists; above, strip height 12 gets a
                    launch of its own beside the other three; 0 .. 2147483647, default 49152, 0 = every band stage takes the large form)
     chain_prio     (stream-ordered orientation stage: wave priority of what runs on the voted strand's side stream beside the other strand's
                    full sweeps.  "0" none, "1" the tiers of the pruned sweep and the early decision, "2" also the early preliminary / final
                    alignments of `tracy align`; any other value is refused; default "1")
   Every option selects another EXACT path (A/B measurements, tests of the fallback tiers); none changes a result.  Lanes inherit.
   TRACYHIP_HOST_THREADS, TRACYHIP_HOST_TIMERS, TRACYHIP_LDS_PAD and TRACYHIP_LDS_STAGE_LIMIT are per process (read once).
   tracyhip_describe writes the current settings as "name=value" lines (at most cap - 1 bytes) and returns the length needed.
   tracyhip_describe_options does so without a context or a device: the options a context created NOW would start with (the defaults and
   the TRACYHIP_* environment) with name = value set on top (name NULL: nothing set); TRACYHIP_ERR_ARG for an option or value that
   tracyhip_set_option would refuse. */
int tracyhip_set_option(tracyhip_ctx* ctx, const char* name, const char* value);
int tracyhip_describe(tracyhip_ctx* ctx, char* buf, size_t cap);
int tracyhip_describe_options(const char* name, const char* value, char* buf, size_t cap);
/* glibc allocator settings that keep the descriptor vectors of the HOST-PLANNED pipelines (no_stream, and the fallback tiers) on the
   heap: M_MMAP_THRESHOLD 32 MB, M_TRIM_THRESHOLD 1 GB, M_TOP_PAD 64 MB.  Process-wide, therefore opt-in: a command-line tool or a
   benchmark calls it once; a library loaded into somebody else's process does not touch the allocator.  (TRACYHIP_MALLOPT=1 in the
   environment does the same at the first tracyhip_create.) */
int tracyhip_tune_host_allocator(void);
/* Which tiers the traces of the last tracyhip_align_traces / tracyhip_decompose_traces call on this context took (summed over its
   lanes).  The pipelines certify every shortcut per trace and repeat what fails on a wider form: these counters say how often. */
typedef struct {
  uint32_t traces;
  uint32_t stream_ordered;       /* 1: planned on the device, one host synchronisation at the end; 0: planned by the host */
  uint32_t host_syncs;           /* host synchronisations of the call */
  uint32_t fallback_traces;      /* stream-ordered call: traces handed to the host-planned tiers afterwards */
  uint32_t pruned;               /* orientation stage: traces whose voted strand took the pruned sweep (front.h) */
  uint32_t pruned_uncertified;   /* ... of which not certified in either tier (swept in full) */
  uint32_t prelim_banded;        /* preliminary alignment on the band kernels */
  uint32_t prelim_repeated;      /* ... of which repeated on the wider form */
  uint32_t final_banded;         /* `tracy align`: final alignments on a certified band */
  uint32_t final_repeated;
  uint32_t allele_pruned[2];     /* `tracy decompose`: gotoh(allele k, window) by the pruned sweep */
  uint32_t allele_uncertified[2];
  uint32_t allele_banded[3];     /* allele k vs its slice (k = 0, 1), allele 1 vs allele 2 (k = 2) on the band kernels */
  uint32_t allele_repeated[3];
  uint32_t allele_shared_prefix; /* stream-ordered `tracy decompose`: traces whose second allele begins with the same 128 characters as the first and
                                    reads the prefix row kept for it (counted in allele_pruned[1] as well) */
  uint32_t cons_fixup_columns;   /* tracyhip_consensus_traces: consensus columns the device screen handed to the host gtLetter */
  uint32_t cons_chunks;          /* ... chunks the batch was cut into to fit the workspace limit */
  uint32_t asm_chunks;           /* tracyhip_assemble_traces: chunks of groups the batch was cut into to fit the workspace limit */
  uint32_t asm_steps;            /* ... chain steps launched, summed over the chunks (a chunk runs as many as its largest group has matching traces) */
  uint32_t denovo_chunks;        /* tracyhip_denovo_traces: chunks of groups the batch was cut into to fit the workspace limit */
  uint32_t denovo_rounds;        /* ... overlap rounds launched, summed over the chunks (a chunk runs as many as its slowest trace tries partners) */
  uint32_t denovo_steps;         /* ... tree heights launched, summed over the chunks (a chunk runs as many as its tallest tree has) */
  uint32_t var_traces;           /* tracyhip_decompose_variants: traces whose variants were called (status 0) */
  uint32_t var_realigned;        /* ... of which on the reverse strand: both alleles re-aligned as reverse complements (indigo.h:408-422) */
  uint32_t var_truncated;        /* ... traces whose events did not fit max_variants / max_text (var_flags bit 0) */
  uint32_t var_chunks;           /* ... chunks of traces the batch was cut into to fit the workspace limit */
  uint32_t sweep_diag_launches;  /* 16-bit full sweeps launched in the offset form (six operations per cell; 0 with no_sweep_diag or where the range rule finds no room) */
  uint32_t prefix_diag_launches; /* ... launches of prefix sweeps in the offset form */
  uint32_t band_list_pairs[2][4]; /* stream-ordered pipelines: pairs the scan of a band stage filed under strip height 12 / 8 / 4 / the quad form, summed
                                     over the call's band stages; [0]: traceback stages, [1]: origin sweeps.  0 in a call planned by the host */
  uint32_t band_large_launches;  /* ... band stages of more than b16_multi_max units: strip height 12 in a launch of its own beside the other three lists */
  uint32_t seed_spilled;         /* tracyhip_seed_traces with seed_spill (which sets these three and no other counter): traces answered by the spill kernel */
  uint32_t seed_spill_launches;  /* ... spill launches the call made (one more synchronisation each) */
  uint32_t seed_spill_deferred;  /* ... spilled traces handed to the host because their tables did not fit the workspace limit */
  uint32_t wt_chunks;            /* tracyhip_align_traces, wildtype job: chunks of traces the batch was cut into to fit the workspace limit (like
                                    every counter summed over the lanes of the call; 0 when the call failed) */
} tracyhip_call_stats;
int tracyhip_last_call_stats(tracyhip_ctx* ctx, tracyhip_call_stats* out);
const char* tracyhip_last_error(void);
const char* tracyhip_version(void);

/* ---- DP ---------------------------------------------------------------------------------------- */
/* gotohScore, gotoh.h:12-68: scores[i] = s[n] of pair i. */
int tracyhip_gotoh_score(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, const tracyhip_params* prm,
                         int mem, int32_t* scores);
/* gotoh, gotoh.h:71-174.  ops receives the reference's `btr` (gotoh.h:147-167): 's','h','v' in PUSH
 * ORDER, i.e. from the end of the alignment to its start; pair i writes ops_len[i] <= m+n bytes at
 * ops + ops_offset[i] (ops_offset is a HOST array).  scores may be NULL. */
int tracyhip_gotoh_align(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, const tracyhip_params* prm,
                         int mem, int32_t* scores, uint8_t* ops, const uint64_t* ops_offset,
                         uint32_t* ops_len);
/* gotoh (gotoh.h:71-174) on a diagonal band chosen by the caller: pair i is swept on the diagonals c - r in [band_lo[i], band_hi[i]]
 * only (the last row on to column n: its free trailing run), cells outside read as -inf.  Scores, `btr` (and ends) are those of
 * tracyhip_gotoh_align whenever the band holds every optimal path, which is the caller's to establish -- e.g. for strings with
 * free horizontal end gaps: a path that leaves [-W - (m-n)+, W + (n-m)+] makes more than W vertical gap steps, so it scores at
 * most match*m - (match + |ge|)(W+1) - |go|; a banded score above that is the optimum.  This is the form the
 * pipelines below use internally for their final alignments.  CHAR x CHAR or PROFILE x CHAR pairs, AlignConfig<hfree,false>,
 * go <= 0, ge < 0, bands of at most 184 diagonals and references of at most ~14 800 columns (the codes of four pairs are staged in
 * LDS; TRACYHIP_ERR_RANGE beyond).  CHAR rows must hold the letters A C G T N only (the kernels score through a five-letter table,
 * so any other byte would mismatch an identical column byte where gotoh.h compares bytes): TRACYHIP_ERR_ARG otherwise -- such
 * strings go through tracyhip_gotoh_align.  Columns may hold any byte (other letters mismatch every row, as in gotoh.h).  A pair whose traceback walk leaves its band reports
 * ops_len 0.  ends != NULL: the origin-tracking sweep instead of the traceback -- scores and ends[2i] = leading 'h' columns,
 * ends[2i+1] = last column that is not a trailing 'h' (what trimReferenceSlice, fmindex.h:429-463, reads); ops* may be NULL then. */
int tracyhip_gotoh_banded(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, const tracyhip_params* prm, const int32_t* band_lo,
                          const int32_t* band_hi, int mem, int32_t* scores, uint8_t* ops, const uint64_t* ops_offset, uint32_t* ops_len,
                          uint32_t* ends);
/* needleScore / needle, needle.h:12-57 / 59-138 (linear gap cost ge; profiles scored in double). */
int tracyhip_needle_score(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, const tracyhip_params* prm,
                          int mem, int32_t* scores);
int tracyhip_needle_align(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, const tracyhip_params* prm,
                          int mem, int32_t* scores, uint8_t* ops, const uint64_t* ops_offset,
                          uint32_t* ops_len);
/* _createAlignment, align.h:196-223 (CHAR) / 254-293 (PROFILE: consensus characters).  For pair i,
 * row0/row1 receive ops_len[i] bytes each at rows0 + ops_offset[i] / rows1 + ops_offset[i]. */
int tracyhip_alignment_rows(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, int mem, const uint8_t* ops,
                            const uint64_t* ops_offset, const uint32_t* ops_len, uint8_t* rows0,
                            uint8_t* rows1);

/* ---- whole `tracy align` hot section (sage.h:191-311) for a batch of traces ---------------------
 * Per trace t:   full profile  P_f = float[6][mf]        (createProfile(tr,bc), sage.h:193)
 *                trimmed profile = columns [trim_left, mf - trim_right) of P_f (sage.h:197; identical
 *                values: createProfile computes each column independently, profile.h:28-51)
 *                reference window  R = bytes[n]           (loadSingleFasta output, sage.h:226)
 * Steps (all on the device): gotohScore(trim, R) and gotohScore(trim, revcomp R) (sage.h:239-240);
 * forward iff gsFwd > gsRev (:247); gotoh(trim, oriented R) (:258); trimReferenceSlice (:259,
 * fmindex.h:429-463); gotoh(full, trimmed slice) (:311). */
typedef struct {
  uint32_t ntraces;
  tracyhip_seqset profiles; /* kind PROFILE, one full profile per trace */
  tracyhip_seqset refs;     /* kind CHAR: reference windows (FASTA / indexed genome).  kind PROFILE: a WILDTYPE job (sage.h:261-300 + :311),
                               the reference of every trace is a second chromatogram -- the FORWARD profile of every distinct wildtype
                               (createProfile(gtr, gbc)), host or device per `mem`; without ref_index count >= ntraces.  See "wildtype
                               jobs" below.  (The struct does not grow for it: its size and every offset are what they were.) */
  const uint32_t* ref_index; /* HOST array or NULL (= identity) */
  uint32_t trim_left;       /* SageConfig.trimLeft  (sage.h:88) */
  uint32_t trim_right;      /* SageConfig.trimRight (sage.h:89) */
  const uint8_t* oriented;  /* HOST array or NULL.  Non-NULL = the indexed-genome path (sage.h:217-221): the caller anchored
                               every trace by k-mer seeding (getReferenceSlice, fmindex.h:236-326) and passes refs that are
                               ALREADY oriented (reverse-complemented for reverse traces); oriented[t] = rs.forward.  No
                               orientation scores are computed: score_fwd and score_rev both receive gotohScore(trim, ref). */
  uint32_t strand_by_certificate; /* 0 (default, what a zero-initialised job gets): both gotohScore calls run in full; score_fwd and
                               score_rev are gsFwd and gsRev.  1 (opt-in): the strand is still decided exactly as the reference
                               does (forward iff gsFwd > gsRev), but the LOSING orientation may be represented by a certified
                               upper bound of its score instead of the score itself (a prefix of its DP suffices to prove that
                               it cannot win; see pipeline.hip) -- fewer cells, same decision, same alignments. */
  const uint32_t* trim_left_each;  /* HOST arrays [ntraces], or both NULL (what a zero-initialised job gets: every trace takes the */
  const uint32_t* trim_right_each; /* scalars above).  Given: trace t uses trim_left_each[t] / trim_right_each[t] wherever the scalars
                               are used, and the scalars are ignored (per-trace trims, below).  One without the other: TRACYHIP_ERR_ARG. */
} tracyhip_align_job;

/* ---- wildtype jobs (tracyhip_align_job::refs of kind PROFILE) ---------------------------------------------------------------------
 * Per trace t with wildtype W (n columns), all on the device and in stream order:
 *   trimmed = columns [l, mf - r) of the full profile (rule 1 of the per-trace trims below; scalars or trim_*_each)
 *   gsFwd = gotohScore(trimmed, W), gsRev = gotohScore(trimmed, revcomp W)   (sage.h:289-290; revcomp once per DISTINCT wildtype)
 *   forward = gsFwd > gsRev: a tie is reverse (sage.h:293)
 *   score_final / ops / ops_len = gotoh(full profile, chosen strand of W), push order, capacity mf + n at ops_offset[t]   (sage.h:311)
 *   rows0 / rows1 (optional) = the _createAlignment rows of that alignment
 * score_fwd / score_rev are both exact: strand_by_certificate is IGNORED for wildtype jobs.  There is no preliminary alignment and no
 * trimReferenceSlice in this branch: score_prelim (if non-NULL) receives the chosen strand's orientation score, slice_begin = 0,
 * slice_len = n, ref_pos = 0.  With `oriented` non-NULL the profiles are taken as already oriented: one score per trace goes into both
 * score_fwd and score_rev (as on the indexed-genome path) and forward[t] = oriented[t].
 * The traceback planes are chunked by traces to the workspace limit (tracyhip_call_stats::wt_chunks); the call synchronises twice
 * (the profile classes, the end) whatever ntraces or the number of chunks is, and twice that when a 16-bit score launch met an
 * un-normalised profile and the call repeats on int32. */

/* ---- per-trace trims (`-t`: trimTrace gives every trace its own trimLeft / trimRight, sage.h:39-40, trim.h:35-73) ----------------
 * tracyhip_align_job, tracyhip_decompose_job (which tracyhip_decompose_variants reads) and tracyhip_seed_params carry two optional
 * HOST arrays beside their scalar pair.  Every rule below is the scalar rule, applied with the trace's own (l, r):
 *   1. trimmed profile: createProfile's clamp (profile.h:24-27): l + r >= mf gives trims 0 / 0.
 *   2. trimReferenceSlice widening (fmindex.h:443-461): takes the REQUESTED (l, r), not the clamped ones.
 *   3. allele strings and allelic fraction: trimmedSeq (abif.h:68-75): l + r + 1 >= len gives the whole string (one off from rule 1).
 *   4. allelic fraction index: bcPos[i + l], clamped to the last basecall (decompose.h:445).
 *   5. decomposeAlleles: nbc - r in size_t arithmetic, breakpoint + l (decompose.h:216).
 *   6. variants: call_index = l + basenum - 1 forward, bc_len - (r + basenum) reverse (variants.h:205).
 *   7. k-mer orientation vote: the profile columns [l, mf - r) of rule 1.
 *   8. seeding: the trace's k-mers from [l, len - r); a trim shorter than k - 1 or a consensus shorter than a trim defers THAT trace.
 * The requested pairs travel to the device inside the per-trace records a call uploads anyway: no further copy, no further
 * synchronisation.  The stage calls (tracyhip_decompose_alleles, tracyhip_allelic_fraction, tracyhip_trim_reference_slice,
 * tracyhip_call_variants) keep their scalar trims. */

typedef struct {
  int32_t* score_fwd;     /* [ntraces] gsFwd (with strand_by_certificate: exact for the winning orientation only) */
  int32_t* score_rev;     /* [ntraces] gsRev (idem) */
  uint8_t* forward;       /* [ntraces] 1 = rs.forward */
  int32_t* score_prelim;  /* [ntraces] score of the preliminary alignment (sage.h:258), may be NULL */
  uint32_t* slice_begin;  /* [ntraces] ri: offset of the trimmed slice in the ORIENTED reference */
  uint32_t* slice_len;    /* [ntraces] length of the trimmed slice (after substr clamping) */
  uint32_t* ref_pos;      /* [ntraces] rs.pos after trimReferenceSlice (rs.pos starts at 0, sage.h:244) */
  int32_t* score_final;   /* [ntraces] score of the final alignment (sage.h:311) */
  uint8_t* ops;           /* final alignment, push order, at ops + ops_offset[t] (capacity mf + slice).  Only the first ops_len[t]
                             bytes are defined: the rest of a trace's region may hold bytes of an alignment that was begun for the
                             voted strand and discarded when the other strand's exact score won */
  const uint64_t* ops_offset; /* HOST array */
  uint32_t* ops_len;      /* [ntraces] */
  uint8_t* rows0;         /* OPTIONAL, both or neither; wildtype jobs only (TRACYHIP_ERR_ARG otherwise).  The _createAlignment rows of the final */
  uint8_t* rows1;         /* alignment (align.h:254-293: consensus characters of the trace profile / of the chosen strand of the wildtype),
                             ops_len[t] bytes each at ops_offset[t].  The chosen strand exists on the device only, so tracyhip_alignment_rows
                             could not give them without the reverse complement being made again */
} tracyhip_align_result;

/* what tracyhip_align_traces checks before it plans, on the host (no device is touched): job / prm / out and the result arrays it
 * always writes non-NULL, `mem` one of the two kinds, ops_offset given, both or neither of trim_left_each / trim_right_each; for a
 * wildtype job (refs of kind PROFILE) a non-NULL payload and, without ref_index, count >= ntraces; rows0 / rows1 both or neither, and
 * neither on a job whose refs are of kind CHAR; any other kind of refs.
 * TRACYHIP_ERR_ARG (with the reason) otherwise.  The compute call runs it first. */
int tracyhip_align_validate(const tracyhip_align_job* job, const tracyhip_params* prm, int mem, const tracyhip_align_result* out);
int tracyhip_align_traces(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm,
                          int mem, const tracyhip_align_result* out);

/* ---- allele deconvolution (`tracy decompose`, indigo.h:190-388) ------------------------------------ */
/* TraceBreakpoint, fmindex.h:51-56 */
typedef struct {
  int32_t indelshift;
  int32_t traceleft;
  uint32_t breakpoint;
  float best_diff;
} tracyhip_breakpoint;

/* Trace + BaseCalls of a batch (abif.h:28-57), flattened.  signal/bcpos/primary/secondary are payloads
 * (host or device per `mem`), the offset/length arrays are HOST arrays. */
typedef struct {
  uint32_t ntraces;
  const int32_t* signal;         /* trace t: channels A,C,G,T at signal + signal_offset[t] + k*nsamples[t] */
  const uint64_t* signal_offset;
  const uint32_t* nsamples;
  const int32_t* bcpos;          /* bc.bcPos of trace t at bcpos + bc_offset[t] */
  uint8_t* primary;              /* bc.primary   at primary   + bc_offset[t] (rewritten by decomposeAlleles) */
  uint8_t* secondary;            /* bc.secondary at secondary + bc_offset[t] (rewritten by decomposeAlleles) */
  const uint64_t* bc_offset;
  const uint32_t* bc_len;        /* bc.consensus.size() */
  const int32_t* peaks;          /* OPTIONAL (NULL = built on the device from signal + bcpos).  The peak table: the four channels at every
                                    basecall's peak position, peaks[4 * (bc_offset[t] + i) + k] = traceACGT[k][bcPos[i]] of trace t (payload, host
                                    or device per `mem`).  Every read of the chromatogram on this path is at a peak position
                                    (generateSecondaryDecomposed decompose.h:378-410, allelicFraction decompose.h:445-470; createProfile
                                    profile.h:21-52 on the host), so a caller that has the trace in hand -- the command line, while it basecalls --
                                    passes 16 bytes per basecall instead of the chromatogram (192 KB per 1 kb trace); signal, signal_offset,
                                    nsamples and bcpos may then be NULL. */
} tracyhip_basecalls;

/* the IndigoConfig fields decomposeAlleles reads (indigo.h:16-40; CLI defaults 50, 50, 1000, 5) */
typedef struct {
  int32_t trim_left;
  int32_t trim_right;
  int32_t maxindel;              /* 1 .. 65536; traces must hold fewer than 131072 basecalls (TRACYHIP_ERR_RANGE beyond).  The scan
                                  * tables of decomposeAlleles are LDS resident up to 4096 / 8191 basecalls (two size classes) and live
                                  * in global memory beyond that (slower, same results) */
  int32_t madc;
} tracyhip_decomp_params;

/* what decomposeAlleles printed / chose: kind 0 = an indel shift was applied, 1 = "Complex mutation,
 * decomposition: ins, del, error" (decompose.h:315), 2 = "No InDel detected" (decompose.h:327) */
typedef struct {
  int32_t kind;
  int32_t best_ins;
  int32_t best_del;
  int32_t best_fr;
  uint32_t dcp_n; /* rows written to the decomposition table */
  uint32_t pad;
} tracyhip_decomp_status;

/* findBreakpoint, decompose.h:7-56: one breakpoint per profile of the set. */
int tracyhip_find_breakpoint(tracyhip_ctx* ctx, const tracyhip_seqset* profiles, int mem, tracyhip_breakpoint* out);
/* findHomozygousBreakpoint, decompose.h:59-128, applied to the traces whose bps[t].indelshift == 0
 * (indigo.h:314-317).  status[t]: 1 ok, 0 "No valid alignment", -1 "Alignment too short". */
int tracyhip_find_homozygous_breakpoint(tracyhip_ctx* ctx, uint32_t ntraces, const uint8_t* rows0, const uint8_t* rows1,
                                        const uint64_t* rows_offset, const uint32_t* rows_len, int mem,
                                        tracyhip_breakpoint* bps, int32_t* status);
/* decomposeAlleles, decompose.h:179-376.  rows0/rows1: the 2-row alignment of the trimmed trace vs the
 * reference slice (tracyhip_alignment_rows); bps: payload array; refslice_len: HOST array (rs.refslice.size()).
 * The decomposition table of trace t (pairs indel, error; decompose.h:273-285) goes to dcp_* + dcp_offset[t],
 * capacity 2*maxindel+2 entries, of which status[t].dcp_n are the table (host arrays: the rest comes back zero; device arrays: untouched). */
int tracyhip_decompose_alleles(tracyhip_ctx* ctx, const tracyhip_basecalls* bc, const uint8_t* rows0, const uint8_t* rows1,
                               const uint64_t* rows_offset, const uint32_t* rows_len, const tracyhip_breakpoint* bps,
                               const uint32_t* refslice_len, const tracyhip_decomp_params* prm, int mem,
                               int32_t* dcp_indel, int32_t* dcp_err, const uint64_t* dcp_offset, tracyhip_decomp_status* status);
/* generateSecondaryDecomposed, decompose.h:378-410: secdecomp + bc_offset[t] receives bc.secDecompose. */
int tracyhip_secondary_decomposed(tracyhip_ctx* ctx, const tracyhip_basecalls* bc, int mem, uint8_t* secdecomp);
/* allelicFraction, decompose.h:412-621: fractions[2t], fractions[2t+1] = the returned pair. */
int tracyhip_allelic_fraction(tracyhip_ctx* ctx, const tracyhip_basecalls* bc, const uint8_t* secdecomp, uint32_t trim_left,
                              uint32_t trim_right, int mem, double* fractions);

/* trimReferenceSlice, fmindex.h:429-463, on the two rows of an alignment of a trace (row 0) against its reference slice
 * (row 1): slice_begin[t] = ri after the trimLeft widening, slice_len[t] = the length rs.refslice.substr(ri, risize) has,
 * ref_pos[t] = what the call adds to rs.pos (ri forward; oldlen - ri - risize reverse, 0 when that is negative -- the
 * reference only warns).  refslice_len (rs.refslice.size()) and forward (rs.forward) are HOST arrays. */
int tracyhip_trim_reference_slice(tracyhip_ctx* ctx, uint32_t ntraces, const uint8_t* rows0, const uint8_t* rows1,
                                  const uint64_t* rows_offset, const uint32_t* rows_len, const uint32_t* refslice_len,
                                  const uint8_t* forward, uint32_t trim_left, uint32_t trim_right, int mem,
                                  uint32_t* slice_begin, uint32_t* slice_len, uint32_t* ref_pos);

/* ---- whole `tracy decompose` hot section (indigo.h:190-388) for a batch of traces, FASTA reference ----
 * findBreakpoint(trimmed profile) -> orientation scores -> gotoh(trimmed, oriented reference) with the
 * score gate of indigo.h:303-309 -> findHomozygousBreakpoint when no shift was seen -> decomposeAlleles ->
 * generateSecondaryDecomposed -> allelicFraction -> per allele: gotoh(seq, rs.refslice), trimReferenceSlice,
 * gotoh(seq, trimmed slice) -> gotoh(primary, secondary) global.  bc.primary / bc.secondary are rewritten
 * in place (decomposed basecalls).  prm->hfree/vfree are ignored (the configs are fixed by indigo.h). */
typedef struct {
  uint32_t ntraces;
  tracyhip_seqset profiles;      /* kind PROFILE: createProfile(tr, bc) of every trace, bc_len[t] columns */
  tracyhip_basecalls bc;
  tracyhip_seqset refs;          /* kind CHAR, upper-case [ACGTN] */
  const uint32_t* ref_index;     /* HOST array or NULL */
  tracyhip_decomp_params dprm;
  const uint8_t* oriented;       /* HOST array or NULL; as in tracyhip_align_job: refs already oriented by k-mer seeding
                                    (indigo.h:213-218), oriented[t] = rs.forward; score_fwd / score_rev are then zero */
  tracyhip_seqset ref_profiles;  /* data NULL = unused.  Wildtype-trace reference (indigo.h:249-289): kind PROFILE, the profile of every
                                    wildtype trace, parallel to refs (same count, same lengths), which then hold the wildtype's primary
                                    basecalls = rs.refslice.  With `oriented`: both already oriented by the caller.  Without: both are
                                    the FORWARD wildtype and the call chooses the strand (indigo.h:276-277): gsFwd / gsRev =
                                    gotohScore(trimmed trace profile, W / revcomp W), forward = gsFwd > gsRev, all three written to
                                    score_fwd / score_rev / forward; everything from indigo.h:302 on runs against the chosen strand (the
                                    reverse complement of the profile, made on the device once per distinct wildtype, and of refs) */
  uint32_t strand_by_certificate; /* as in tracyhip_align_job: 0 (default) = both orientation scores exact; 1 = the losing
                                    orientation's score may be a certified upper bound */
  const uint32_t* trim_left_each;  /* HOST arrays [ntraces], or both NULL: as in tracyhip_align_job, in place of dprm.trim_left / */
  const uint32_t* trim_right_each; /* dprm.trim_right.  A value above INT32_MAX is TRACYHIP_ERR_ARG (a negative trim, per trace). */
} tracyhip_decompose_job;

typedef struct {
  tracyhip_breakpoint* bp;       /* [ntraces] breakpoint used by decomposeAlleles */
  int32_t* status;               /* [ntraces] 0 ok; -1 "Alignment of trace to reference failed!" (indigo.h:306-309);
                                    findHomozygousBreakpoint failed (:316): -2 "No valid alignment found ..." (decompose.h:81),
                                    -3 "Alignment too short ..." (:92).  Later outputs of such traces are unspecified. */
  int32_t* score_fwd;
  int32_t* score_rev;
  uint8_t* forward;
  int32_t* score_trim;           /* aliTrimScore (indigo.h:302) */
  int32_t* dcp_indel;            /* decomposition table, trace t at dcp_offset[t], capacity 2*maxindel+2 */
  int32_t* dcp_err;
  const uint64_t* dcp_offset;    /* HOST array */
  tracyhip_decomp_status* dstatus;
  uint8_t* secdecomp;            /* bc.secDecompose, trace t at bc.bc_offset[t] */
  double* fractions;             /* [2*ntraces] allelicFraction */
  /* allele alignments k = 0 (primary vs its trimmed slice), 1 (secondary), 2 (primary vs secondary, global);
   * ops in push order, capacity len(seq) + len(reference) (k < 2) or 2*len(seq) (k = 2) */
  uint32_t* slice_begin[2];
  uint32_t* slice_len[2];
  uint32_t* ref_pos[2];
  int32_t* score[3];
  uint8_t* ops[3];
  const uint64_t* ops_offset[3]; /* HOST arrays */
  uint32_t* ops_len[3];
} tracyhip_decompose_result;

/* what tracyhip_decompose_traces checks before it plans, on the host (no device is touched): NULL arguments and result arrays,
 * `mem`, the basecall arrays, maxindel (TRACYHIP_ERR_RANGE), both or neither of the per-trace trim arrays and their range.
 * With ref_profiles: its kind, offset / length arrays, the same count and lengths as refs, and count >= ntraces without ref_index.
 * TRACYHIP_ERR_ARG (with the reason) otherwise.  The compute call runs it first. */
int tracyhip_decompose_validate(const tracyhip_decompose_job* job, const tracyhip_params* prm, int mem, const tracyhip_decompose_result* out);
int tracyhip_decompose_traces(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_params* prm, int mem,
                              const tracyhip_decompose_result* out);

/* ---- variant calling of `tracy decompose -v` (indigo.h:397-443 over variants.h:34-126) -----------------------------------
 * One variant of a trace: what the reference's Variant holds, with the basecall it sits on.  ref is the ref_len bytes at
 * text + t * max_text + ref_off, alt the alt_len bytes at ... + alt_off (no terminators; offsets into the trace's OWN text region).
 * gt: 1 = seen on one allele ("0/1"), 2 = the same (pos, ref, alt) on both ("1/1").  call_index = variantCallIndex (variants.h:205):
 * forward traces trim_left + basenum - 1, reverse traces bc_len - (trim_right + basenum) -- the index of estQual / bcPos the writers read. */
typedef struct {
  int32_t pos;
  int32_t basenum;
  int32_t gt;
  uint32_t call_index;
  uint32_t ref_off;
  uint32_t ref_len;
  uint32_t alt_off;
  uint32_t alt_len;
} tracyhip_variant;

/* callVariants (variants.h:56-126) of both allele alignments of every trace, insertVariant (:34-53) across the two, the sort of
 * indigo.h:442 and variantCallIndex.  rows0 / rows1 / rows_offset / rows_len describe 2 * ntraces two-row alignments as
 * tracyhip_trim_reference_slice takes them (row 0 the allele, row 1 its reference slice); alignments 2t and 2t + 1 are allele 1 and
 * allele 2 of trace t.  HOST arrays: pos[2 * ntraces] (rs.pos of each alignment), forward[ntraces], bc_len[ntraces]
 * (bc.primary.size()).  max_variants in 1 .. 1024 (TRACYHIP_ERR_RANGE beyond), max_text in bytes.
 * Results where `mem` says: trace t's records at var + t * max_variants, its text at text + t * max_text, var_n[t] records.
 *   - Order: by (pos, basenum); ties -- which Variant::operator< leaves open -- allele 1's events before allele 2's, each allele in
 *     the order callVariants pushes them.  That is what std::stable_sort gives the host writers.
 *   - Text: record r's ref then its alt, records back to back from offset 0.
 *   - A trace whose events do not fit (more than max_variants on either allele or after the merge, or more than max_text bytes of
 *     ref + alt) returns var_n[t] = 0 and var_flags[t] = 1 (0 otherwise); the call still returns TRACYHIP_OK.
 *   - Of var and text only the first var_n[t] records of a trace and the text bytes they point to are ever written, in both kinds of
 *     `mem`: with host arrays everything else in the caller's arrays keeps the bytes it had. */
int tracyhip_call_variants(tracyhip_ctx* ctx, uint32_t ntraces, const uint8_t* rows0, const uint8_t* rows1, const uint64_t* rows_offset,
                           const uint32_t* rows_len, const int32_t* pos, const uint8_t* forward, const uint32_t* bc_len, uint32_t trim_left,
                           uint32_t trim_right, uint32_t max_variants, uint32_t max_text, int mem, tracyhip_variant* var, uint8_t* text,
                           uint32_t* var_n, uint32_t* var_flags);

/* the four result arrays of the two calls, with their capacities per trace */
typedef struct {
  tracyhip_variant* var;   /* [ntraces * max_variants] */
  uint8_t* text;           /* [ntraces * max_text] */
  uint32_t* var_n;         /* [ntraces] */
  uint32_t* var_flags;     /* [ntraces] bit 0: truncated */
  uint32_t max_variants;   /* 1 .. 1024 */
  uint32_t max_text;       /* >= 2 */
} tracyhip_variants_result;

/* indigo.h:397-423, 442-443 for a batch: the variant list of every trace of a tracyhip_decompose_traces call.  job: the job of that
 * call; res: the result it filled (same `mem`; bp, scores, tables and fractions are not read); slice_pos: HOST array [ntraces], rs.pos
 * of each trace's reference window (0 for a single FASTA); prm: the scoring of that call (hfree / vfree ignored).
 *   - status[t] != 0: var_n[t] = 0.
 *   - forward traces: the rows of allele alignment k = 0, 1 from ops[k], the trimmed primary / secdecomp and
 *     oriented reference[slice_begin[k] .. + slice_len[k]); pos = slice_pos[t] + ref_pos[k][t].
 *   - reverse traces (indigo.h:408-422): reverseComplement of the trimmed allele and of its slice (letters outside ACGTNacgtn keep the
 *     byte of their OUTPUT position, as the reference's table leaves them), gotoh(rc allele, rc slice) semi-global with free horizontal
 *     ends through the internal path of tracyhip_gotoh_align -- all reverse traces of a chunk as one batch of pairs --, then rows and
 *     scan with the same pos.
 * Results as tracyhip_call_variants describes them.  The batch is cut into chunks of consecutive traces whose rows, reverse
 * complements and op strings fit the workspace limit (tracyhip_set_workspace_limit); the traceback planes of a chunk's
 * re-alignments are planned under the same limit by the DP driver, on top of that.  Host synchronisations
 * (tracyhip_call_stats::host_syncs):
 *     the number of chunks BEFORE THE LAST that hold a usable reverse trace   (such a chunk is waited for behind its scan: the
 *                                                     traceback batch of the next one reuses the context's descriptor staging)
 *   + TRACYHIP_MEM_DEVICE: 1 (one read of forward / status / slice_* / ref_pos / ops_len, from which the host plans) + 1 (the end)
 *     TRACYHIP_MEM_HOST:   1 (counts, flags and where the packed records begin) + 1 (the packed records and text; not when no trace
 *                          has a variant) -- the plan is read from the caller's arrays
 * -- two for a call of one chunk, at most one more per further chunk, whatever ntraces is. */
int tracyhip_decompose_variants_validate(const tracyhip_decompose_job* job, const tracyhip_decompose_result* res, const uint32_t* slice_pos,
                                         const tracyhip_params* prm, int mem, const tracyhip_variants_result* out);
int tracyhip_decompose_variants(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_decompose_result* res,
                                const uint32_t* slice_pos, const tracyhip_params* prm, int mem, const tracyhip_variants_result* out);

/* ---- k-mer seeding in an indexed genome (getReferenceSlice, fmindex.h:236-326) on the device ----------------------------
 * The index is tracy_amd/host/seed.hpp's GenomeIndex (tracyhost_genome_view gives its arrays): every k-mer over ACGT of the text is
 * filed under the smaller of its code and its reverse complement's; the table is sorted by bucket (the low bucket_bits bits of that
 * code), code, strand part, position; dir[b] .. dir[b + 1] is bucket b's range of the table. */
typedef struct {
  uint32_t k;                /* 1 .. 32 */
  uint32_t bucket_bits;      /* <= min(2k, 24) */
  const uint64_t* dir;       /* [2^bucket_bits + 1], monotone, dir[0] = 0, last = ntab */
  const uint64_t* tab;       /* [2 * ntab]: {code, pos} pairs; bit 63 of pos set: the text holds the code's reverse complement there */
  uint64_t ntab;
  const char* text;          /* the upper-cased contigs joined by '\n' */
  uint64_t text_len;
  const uint64_t* starts;    /* [ncontigs] offset of contig i in the text */
  const uint32_t* lengths;   /* [ncontigs] */
  uint32_t ncontigs;         /* >= 1 */
  const uint32_t* contig_id; /* [ncontigs] or NULL (= identity): the contig index reported for a hit in contig i (the first contig
                                with contig i's name: tracyhost_seed_batch's convention for duplicate names) */
} tracyhip_genome_desc;
typedef struct tracyhip_genome tracyhip_genome;
/* Checks a descriptor on the host (no device is touched): k in 1 .. 32, bucket_bits <= min(2k, 24), a monotone directory from 0 to
 * ntab, contigs inside the text in order, contig_id entries < ncontigs.  TRACYHIP_ERR_ARG (with the reason) otherwise. */
int tracyhip_genome_validate(const tracyhip_genome_desc* desc);
/* validates (tracyhip_genome_validate), then copies the arrays once into device memory owned by the handle (all HOST pointers) */
int tracyhip_genome_upload(tracyhip_ctx* ctx, const tracyhip_genome_desc* desc, tracyhip_genome** genome);
int tracyhip_genome_free(tracyhip_genome* genome);
/* device bytes the handle holds */
uint64_t tracyhip_genome_bytes(const tracyhip_genome* genome);
/* Checks a descriptor a table is to be built from, on the host (no device is touched): k in 1 .. 32, bucket_bits <= min(2k, 24), dir and
 * tab NULL and ntab 0, contigs inside the text in order, contig_id entries < ncontigs.  TRACYHIP_ERR_ARG (with the reason) otherwise. */
int tracyhip_genome_validate_text(const tracyhip_genome_desc* desc);
/* GenomeIndex::build on the device: validates (tracyhip_genome_validate_text), copies the text and contig table once, then builds dir and
 * tab on the device of `ctx` -- word for word what the host builds for the same text, k and bucket_bits (tracyhost_default_bucket_bits(k)
 * is the host's choice).  The handle is one tracyhip_genome_upload would give: tracyhip_seed_traces, _bytes and _free take it.  Device
 * temporaries are freed before the call returns; TRACYHIP_ERR_OOM when device memory runs out (nothing is left allocated). */
int tracyhip_genome_build(tracyhip_ctx* ctx, const tracyhip_genome_desc* desc, tracyhip_genome** genome);
/* table entries of a device genome (built or uploaded) */
int tracyhip_genome_ntab(const tracyhip_genome* genome, uint64_t* ntab);
/* copies the device directory and table to HOST arrays in the tracyhip_genome_desc layout: dir [2^bucket_bits + 1], tab [2 * ntab] */
int tracyhip_genome_download(const tracyhip_genome* genome, uint64_t* dir, uint64_t* tab);

#define TRACYHIP_SEED_UNANCHORED 0
#define TRACYHIP_SEED_ANCHORED 1
#define TRACYHIP_SEED_DEFERRED 2 /* outside what the device answers: seed the trace on the host (tracyhost_seed_batch) */

/* the argument meanings of tracyhost_seed_batch; each value is truncated to 16 bits as SageConfig holds it */
typedef struct {
  uint32_t trim_left;
  uint32_t trim_right;
  uint32_t kmer;             /* must be the index's k (every trace is deferred otherwise) */
  uint32_t min_support;
  uint32_t maxindel;
  const uint32_t* trim_left_each;  /* HOST arrays [consensus->count], or both NULL: trace t's own trims in place of the scalars above, */
  const uint32_t* trim_right_each; /* each value truncated to 16 bits like them (per-trace trims, above); the deferral rules (a trim
                                      shorter than k - 1, a consensus shorter than a trim) are then decided per trace */
} tracyhip_seed_params;

/* per trace t: status[t] (TRACYHIP_SEED_*); for anchored traces forward, kmersupport, pos (window start in the contig), contig and
 * the ORIENTED window, slice_len[t] bytes at slices + t * slice_cap (at most slice_cap) -- the layout tracyhost_seed_batch fills.
 * status, forward, kmersupport, pos, contig and slice_len are HOST arrays; slices is payload (where `mem` says).  Traces that are not
 * anchored get status and slice_len = 0 only; the other fields (and window bytes past slice_len) are left as they were. */
typedef struct {
  int32_t* status;
  uint8_t* forward;
  uint32_t* kmersupport;
  uint32_t* pos;
  uint32_t* contig;
  uint32_t* slice_len;
  uint8_t* slices;
  uint64_t slice_cap;
} tracyhip_seed_result;

/* getReferenceSlice (fmindex.h:236-326, the one-pass form of tracy_amd/host/seed.hpp scanBothStrands) for a batch of consensus strings
 * (kind CHAR; offsets / lengths HOST arrays, bytes where `mem` says).  Results are identical to tracyhost_seed_batch's for every trace
 * the device answers.  DEFERRED: letters other than A C G T N among the windows, |consensus| + k >= 65536, a trim shorter than k - 1,
 * a consensus shorter than a trim, a kmer that is not the index's, or more votes on one strand in one pass than the option
 * seed_vote_cap allows (default and maximum 2048: the vote lists live in LDS).
 * With the option seed_spill = 1 that last reason is gone: a trace over seed_vote_cap -- an amplicon in a gene family or an interspersed
 * repeat, a trace of more than ~2 100 windows -- is answered on the device by a second launch that counts its votes in hash tables in
 * device memory (16 bytes per slot, at least two slots per vote of the larger pass, per strand), with the same results.  The tables
 * of a launch are sized within the workspace limit (tracyhip_set_workspace_limit), spilled traces running in several launches where it
 * is tight; only a trace whose own tables exceed the limit is still DEFERRED.  tracyhip_last_call_stats: seed_spilled,
 * seed_spill_launches, seed_spill_deferred.  A batch without such a trace costs what it costs with the option off. */
int tracyhip_seed_traces(tracyhip_ctx* ctx, const tracyhip_genome* genome, const tracyhip_seqset* consensus, const tracyhip_seed_params* prm,
                         int mem, const tracyhip_seed_result* out);

/* ---- two-trace consensus (`tracy consensus`, consensus.h:501-577) for a batch of trace pairs -----------------------------
 * Per pair i:  first[i]  = createProfile(tr1, bc1, ., trimLeft1, trimRight1), the trimmed profile of trace 1
 *              second[i] = the trimmed FORWARD profile of trace 2; its reverse complement (profile.h:74-90) is made on the device
 * Steps (all on the device): gotohScore(first, second) and gotohScore(first, revcomp) (gsFwd / gsRev); forward iff gsFwd > gsRev
 * (consensus.h:545); gotoh(first, chosen) and its _createAlignment rows; numAligned / numMatch and the overlap test (:540-549:
 * NO_OVERLAP when numAligned < min_overlap or numMatch / numAligned < match_fraction, compared in double); pairwiseConsensus with
 * gtLetter per column (consensus.h:94-171, 189-238).  Letters and qualities are those of the host gtLetter bit for bit: columns whose
 * device log10 could decide differently are screened and recomputed by the host before the call returns.
 * prm: any scoring tracyhip_gotoh_align accepts; the command uses {match, mismatch, go, ge, 1, 1} (AlignConfig<true,true>). */
#define TRACYHIP_CONS_OK 0
#define TRACYHIP_CONS_NO_OVERLAP 1
typedef struct {
  uint32_t npairs;
  tracyhip_seqset first;     /* kind PROFILE, pair i = profile i (count >= npairs, every length >= 1) */
  tracyhip_seqset second;    /* kind PROFILE, forward strand */
  uint32_t compute_union;    /* ConsensusConfig computeUnion (1: unaligned columns of either trace are kept; 0: -i, intersection) */
  uint32_t iupac;            /* useIUPAC (-a) */
  uint32_t min_overlap;      /* minOverlap (-c, default 25) */
  float match_fraction;      /* matchFraction (-f, default 0.5), promoted to double for the comparison */
} tracyhip_consensus_job;

/* per-pair arrays and payloads where `mem` says; offset is a HOST array.  Pair i owns m + n elements (m, n = its two profile lengths) of
 * rows0, rows1, cons and qual from offset[i] on.  A NO_OVERLAP pair gets its scores, rows and counts, and cons_len 0. */
typedef struct {
  int32_t* score_fwd;        /* [npairs] gsFwd */
  int32_t* score_rev;        /* [npairs] gsRev */
  uint8_t* forward;          /* [npairs] 1 = gsFwd > gsRev */
  int32_t* score;            /* [npairs] score of gotoh(first, chosen strand) */
  uint32_t* num_aligned;     /* [npairs] columns with a letter in both rows */
  uint32_t* num_match;       /* [npairs] ... of which equal */
  int32_t* status;           /* [npairs] TRACYHIP_CONS_OK / TRACYHIP_CONS_NO_OVERLAP */
  uint8_t* rows0;            /* _createAlignment row of first, ops_len[i] bytes at offset[i] */
  uint8_t* rows1;            /* ... of the chosen strand of second */
  uint32_t* ops_len;         /* [npairs] alignment columns */
  uint8_t* cons;             /* consensus letters, cons_len[i] bytes at offset[i] */
  uint16_t* qual;            /* their qualities (gq <= 10000), cons_len[i] values at offset[i] */
  uint32_t* cons_len;        /* [npairs] */
  const uint64_t* offset;    /* HOST array */
} tracyhip_consensus_result;

int tracyhip_consensus_traces(tracyhip_ctx* ctx, const tracyhip_consensus_job* job, const tracyhip_params* prm, int mem,
                              const tracyhip_consensus_result* out);

/* ---- basecalling of raw chromatograms (what every command runs first) for a batch of traces --------------------------------
 * Per trace, from the four channels of the chromatogram and the file's call positions (Trace::traceACGT, Trace::basecallpos, abif.h:28-43):
 *   basecall(tr, bc, sigratio)             abif.h:408-511 (window peaks abif.h:77-97): primary / secondary / consensus letters, bcPos
 *   estimateQualities(bc)                  abif.h:232-253 over findBestTraceSection abif.h:164-220: estQual
 *   findBestTraceSection(bc)               abif.h:222-229: best_section (what nearestSNP, trim.h:10-33, starts from)
 *   trimTrace(stringency, bc, l, r)        trim.h:35-73, when trim_stringency is not 0
 *   createProfile(tr, bc, p)               profile.h:21-52: the untrimmed profile float[6][bc_len]
 *   the peak table                         peaks[4 * i + k] = traceACGT[k][bcPos[i]] (tracyhip_basecalls::peaks)
 * A window of two equal borders gives no basecall (abif.h:80), so bc_len[t] <= npos[t]; the results of a trace are packed from the start of
 * its region.  Every result equals the host chain's (tracy_amd/host/tracy_host.hpp, sage_out.hpp) bit for bit, the profile's floats included.
 * The reference indexes the chromatogram unchecked; the device answers a trace only when npos is in 1 .. 131071, nsamples in 3 .. 2^23 and
 * the positions are non-decreasing inside [0, nsamples).  Any other trace is DEFERRED: status and bc_len = 0 are written, nothing else, and
 * the caller runs the host chain for it (the convention of tracyhip_seed_traces). */
#define TRACYHIP_BASECALL_OK 0
#define TRACYHIP_BASECALL_DEFERRED 1 /* outside what the device answers: basecall the trace on the host */
typedef struct {
  uint32_t ntraces;
  const void* signal;            /* payload: int32_t or int16_t samples; trace t: channels A,C,G,T at element signal_offset[t] + k*nsamples[t]
                                    (the layout of tracyhip_basecalls::signal) */
  const uint64_t* signal_offset; /* HOST array, elements */
  const uint32_t* nsamples;      /* HOST array */
  uint32_t sample_bytes;         /* 4: int32_t (what the readers produce); 2: int16_t (what ABIF DATA9..12 stores: half the upload) */
  const int32_t* basecallpos;    /* payload: Trace::basecallpos of trace t at basecallpos + pos_offset[t] */
  const uint64_t* pos_offset;    /* HOST array */
  const uint32_t* npos;          /* HOST array */
  float sigratio;                /* -p, default 0.33 */
  float trim_stringency;         /* -t: 0 = no trimming (trim_left = trim_right = 0), else clamped to 1 .. 9 as the commands do */
} tracyhip_basecall_job;

/* Payload results (where `mem` says; each may be NULL = not wanted): trace t owns npos[t] entries from pos_offset[t] on (peaks: 4 per entry,
 * from 4 * pos_offset[t]; profiles: 6 * npos[t] floats from 6 * pos_offset[t], element (k, j) at k * bc_len[t] + j, rows 4 and 5 zero), of
 * which the first bc_len[t] are written.  Per-trace results are HOST arrays [ntraces] and required.  With TRACYHIP_MEM_DEVICE the payloads
 * are, as they stand, the `profiles` set of tracyhip_align_job / tracyhip_consensus_job / tracyhip_decompose_job (offset 6 * pos_offset[t],
 * length bc_len[t]) and the bcpos / primary / secondary / peaks of tracyhip_basecalls (bc_offset = pos_offset, bc_len). */
typedef struct {
  int32_t* status;        /* TRACYHIP_BASECALL_* */
  uint32_t* bc_len;       /* bc.primary.size() */
  uint32_t* trim_left;    /* trimTrace's leftTrim, truncated to 16 bits as SageConfig holds it (sage.h:39-40) */
  uint32_t* trim_right;
  uint32_t* best_section; /* findBestTraceSection(bc) */
  uint8_t* primary;
  uint8_t* secondary;
  uint8_t* consensus;
  int32_t* bcpos;
  uint8_t* estqual;
  int32_t* peaks;
  float* profiles;
} tracyhip_basecall_result;

/* what tracyhip_basecall_traces checks before it touches a device (none is needed here): NULL job / result / required arrays, mem,
 * sample_bytes other than 2 or 4, a sigratio or trim_stringency that is not a number, a negative trim_stringency, misaligned payloads.
 * TRACYHIP_ERR_ARG (with the reason) otherwise TRACYHIP_OK. */
int tracyhip_basecall_validate(const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out);
/* One launch and ONE host synchronisation per call with device payloads (bc_len is metadata the caller needs on the host to build the next
 * job); host payloads are staged in chunks of consecutive traces whose chromatogram fits the workspace limit (tracyhip_set_workspace_limit;
 * 256 MB without one), with a second synchronisation each for the copy back; the results are the same for any limit.  A trace whose
 * signal_offset + 4 * nsamples or pos_offset + npos leaves 64 bits is refused with TRACYHIP_ERR_RANGE (the error names the trace) before
 * the first launch: nothing is written. */
int tracyhip_basecall_traces(tracyhip_ctx* ctx, const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out);

/* ---- gapped chromatograms: a batch of traces re-spaced along their alignment rows (the last step of `tracy align`, sage.h:321, and
 * the per-trace output step of both assemble modes, assemble.h:352-368, 527-542) ------------------------------------------------
 * Per trace t, in this order:
 *   trimTrace(tr, bc, l, r, nbc)           trim.h:77-99, with trim_left_each / trim_right_each: the basecalls [l, bc_len - r) are kept,
 *                                          the chromatogram is untouched
 *   reverseComplementTrace                 trim.h:125-150 (letters trim.h:102-123), where reverse[t] != 0: sample x -> ns - 1 - x, channel
 *                                          k -> 3 - k, the kept calls in reverse order with bcPos -> ns - 1 - bcPos; estQual travels with
 *                                          its call (Trace::qual is not produced)
 *   alignmentTracePadding(row, ...)        json.h:383-472 along the trace's own row of an alignment (only '-' against anything else is
 *                                          read): every gap run between two letters inserts gap-many pseudo calls ('-', quality 0) of
 *                                          `step` samples of -99 each; the runs at the ends are counted in leading_gaps / trailing_gaps
 * Every field equals tracy_amd/host (assemble_out.hpp, sage_out.hpp alignmentTracePadding).  The device answers a trace when bc_len is in
 * 1 .. 131071, nsamples in 1 .. 2^23, the positions (trimmed ones included) are strictly increasing inside [0, nsamples), l + r < bc_len,
 * the row holds at most as many letters as calls are kept and the padded sizes stay below 2^31.  Any other trace is DEFERRED: status and
 * zero sizes are written, nothing else, and the caller runs the host chain (the convention of tracyhip_basecall_traces).
 * Rows are addressed by row_offset / row_len, so the rows of tracyhip_align_result::rows0 (ops_offset, ops_len), of
 * tracyhip_alignment_rows and row r of group g of an assemble / de novo result (rows_offset[g] + r * ncol[g], ncol[g]) are taken as
 * they stand. */
#define TRACYHIP_PAD_OK 0
#define TRACYHIP_PAD_DEFERRED 1
#define TRACYHIP_PAD_TOO_SMALL 2 /* a capacity is too small: the sizes are reported, no payload is written */
typedef struct {
  uint32_t ntraces;
  const void* signal;            /* payload, as tracyhip_basecall_job (may be NULL where the padded signal is not wanted) */
  const uint64_t* signal_offset; /* HOST array, elements */
  const uint32_t* nsamples;      /* HOST array */
  uint32_t sample_bytes;         /* 4 or 2: of signal here and in the result */
  const int32_t* bcpos;          /* payload, as tracyhip_basecall_result: trace t owns bc_len[t] entries from bc_offset[t] on */
  const uint8_t *primary, *secondary, *consensus, *estqual; /* payload; each needed only where its result is wanted */
  const uint64_t* bc_offset;     /* HOST array */
  const uint32_t* bc_len;        /* HOST array */
  const uint8_t* rows;           /* payload: the row of trace t is row_len[t] bytes from row_offset[t] on */
  const uint64_t* row_offset;    /* HOST array */
  const uint32_t* row_len;       /* HOST array */
  const uint32_t *trim_left_each, *trim_right_each; /* HOST arrays, both or neither; NULL = no hard trim */
  const uint8_t* reverse;        /* HOST array or NULL */
} tracyhip_pad_job;
/* The six per-trace arrays are HOST [ntraces] and required.  The payload results live where `mem` says and each may be NULL.  With all of
 * them NULL the call is the sizes-only form: it needs no offsets or capacities, reads no chromatogram and fills the per-trace arrays
 * (step depends on bcpos, which may live on the device only: this is how a caller sizes its buffers). */
typedef struct {
  int32_t* status;         /* TRACYHIP_PAD_* */
  uint32_t* nsamples_out;  /* samples per channel of the padded trace */
  uint32_t* ncalls_out;    /* calls and pseudo calls */
  uint32_t* leading_gaps;
  uint32_t* trailing_gaps;
  uint32_t* step;          /* samples per pseudo call */
  void* signal;            /* sample_bytes as the job; trace t: channel k at sample_offset[t] + k * nsamples_out[t] */
  const uint64_t* sample_offset; /* HOST array, elements */
  const uint32_t* sample_cap;    /* HOST array: samples per channel that trace t may take (4 * sample_cap[t] elements are its region) */
  int32_t* bcpos;
  uint8_t *primary, *secondary, *consensus, *estqual;
  const uint64_t* call_offset;   /* HOST array */
  const uint32_t* call_cap;      /* HOST array */
} tracyhip_pad_result;
/* what tracyhip_pad_traces refuses before it touches a device (none is needed here): NULL job / result / required arrays, mem,
 * sample_bytes other than 2 or 4, misaligned signal / bcpos, one trim array without the other, a payload result without its offsets and
 * capacities or without its input.  TRACYHIP_ERR_ARG (with the reason) otherwise TRACYHIP_OK. */
int tracyhip_pad_validate(const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out);
/* Device payloads: ONE host synchronisation per call.  Host payloads are staged in chunks of consecutive traces within the workspace
 * limit (tracyhip_set_workspace_limit; 256 MB without one), with a second synchronisation each for the copy back of exactly what was
 * reported. */
int tracyhip_pad_traces(tracyhip_ctx* ctx, const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out);
/* counters of the last tracyhip_pad_traces call of a context.  (A struct of their own: the layout of tracyhip_call_stats is pinned.) */
typedef struct {
  uint32_t pad_chunks;    /* chunks of traces the batch was cut into */
  uint32_t pad_deferred;  /* traces with TRACYHIP_PAD_DEFERRED */
  uint32_t pad_too_small; /* traces with TRACYHIP_PAD_TOO_SMALL */
} tracyhip_pad_stats;
int tracyhip_last_pad_stats(tracyhip_ctx* ctx, tracyhip_pad_stats* out);

/* ---- the text of a batch of traces: what the three writers of the commands print per trace, byte for byte (tracy_amd/host trace_io.hpp
 * traceTxtOut, indigo_out.hpp traceJsonBody, sage_out.hpp assemblyTrace) ----------------------------------------------------------
 * The chromatograms and basecall arrays are read where they lie: the payloads of tracyhip_basecall_result (bc_offset = pos_offset,
 * bc_len) and of tracyhip_pad_result (signal_offset = sample_offset, nsamples = nsamples_out, bc_offset = call_offset, bc_len =
 * ncalls_out) are taken as they stand.  Integers are decimal with a leading '-'; the letters are printed as the bytes they are.
 * The device answers a trace when bc_len is in 1 .. 131071, nsamples in 1 .. 2^23 and the positions are strictly increasing inside
 * [0, nsamples) (the reference's cursor loop then visits every call; its text stays below 2^31 bytes).  Any other trace is DEFERRED:
 * status and text_len = 0 are written, nothing else. */
#define TRACYHIP_RENDER_TSV    0 /* traceTxtOut, abif.h:513-533: the whole file, header line included */
#define TRACYHIP_RENDER_JSON   1 /* _traceJsonOut, json.h:37-105: from "\"pos\": [" through the secondarySeq line and its '\n' */
#define TRACYHIP_RENDER_GAPPED 2 /* assemblyTrace, json.h:130-192: from "\"peakA\": [" through "\"basecalls\": {...}\n"; the lines before
                                    it (file name, leadingGaps, trailingGaps) and the closing "}\n" stay with the caller */
#define TRACYHIP_RENDER_OK 0
#define TRACYHIP_RENDER_DEFERRED 1
#define TRACYHIP_RENDER_TOO_SMALL 2 /* text_cap is too small: text_len is reported, no text is written */
typedef struct {
  uint32_t ntraces, form;
  const void* signal;            /* payload, as tracyhip_pad_job: trace t, channel k at signal_offset[t] + k * nsamples[t] */
  const uint64_t* signal_offset; /* HOST array, elements */
  const uint32_t* nsamples;      /* HOST array */
  uint32_t sample_bytes;         /* 4 or 2 */
  const int32_t* bcpos;          /* payload: trace t owns bc_len[t] entries from bc_offset[t] on, here and in the four below */
  const uint8_t *primary, *secondary, *consensus, *estqual; /* payload; consensus: TSV only (may be NULL otherwise) */
  const uint64_t* bc_offset;     /* HOST array */
  const uint32_t* bc_len;        /* HOST array */
  const uint32_t *trim_left_each, *trim_right_each; /* HOST, both or neither, TSV only: the leftTrim / rightTrim of the trim column; NULL = 0 / 0 */
} tracyhip_render_job;
typedef struct {
  int32_t* status;             /* HOST [ntraces], required: TRACYHIP_RENDER_* */
  uint32_t* text_len;          /* HOST [ntraces], required */
  uint8_t* text;               /* payload: trace t writes exactly text_len[t] bytes from text_offset[t] on; NULL = sizes only */
  const uint64_t* text_offset; /* HOST array, bytes, any value: the text is not aligned */
  const uint64_t* text_cap;    /* HOST array: bytes trace t may take */
} tracyhip_render_result;
/* what tracyhip_render_traces refuses before it touches a device (none is needed here): NULL job / result / required arrays, mem, form,
 * sample_bytes other than 2 or 4, misaligned signal / bcpos, one trim array without the other, a TSV without consensus, a text without its
 * offsets and capacities.  TRACYHIP_ERR_ARG (with the reason) otherwise TRACYHIP_OK. */
int tracyhip_render_validate(const tracyhip_render_job* job, int mem, const tracyhip_render_result* out);
/* Three launches (count the bytes of every tile, scan them per trace, emit), the first two alone in the sizes-only form, which reads the
 * chromatograms too.  Device payloads: ONE host synchronisation per call.  Host payloads are staged in chunks of consecutive traces within
 * the workspace limit (tracyhip_set_workspace_limit; 256 MB without one), with a second synchronisation each for the copy back of exactly
 * the bytes that were reported. */
int tracyhip_render_traces(tracyhip_ctx* ctx, const tracyhip_render_job* job, int mem, const tracyhip_render_result* out);
/* an upper bound of text_len for a trace of these sizes, whatever its values; needs no device.  0: no such form. */
uint64_t tracyhip_render_bound(uint32_t form, uint32_t nsamples, uint32_t bc_len, uint32_t sample_bytes);
/* counters of the last tracyhip_render_traces call of a context.  (A struct of their own: the layout of tracyhip_call_stats is pinned.) */
typedef struct {
  uint32_t render_chunks;    /* chunks of traces the batch was cut into */
  uint32_t render_deferred;  /* traces with TRACYHIP_RENDER_DEFERRED */
  uint32_t render_too_small; /* traces with TRACYHIP_RENDER_TOO_SMALL */
} tracyhip_render_stats;
int tracyhip_last_render_stats(tracyhip_ctx* ctx, tracyhip_render_stats* out);

/* ---- the text of a batch of alignments: what the writers of `align` and `decompose` print from the two gapped rows, byte for byte
 * (tracy_amd/host sage_out.hpp plotAlignment, alignFastaOut, the tail of traceAlignJsonOut) -- where tracyhip_render_traces' GAPPED form
 * stops ------------------------------------------------------------------------------------------------------------------------
 * Alignment i owns cols[i] bytes of rows0 and of rows1 from rows_offset[i] on: the rows of tracyhip_align_result (ops_offset, ops_len) and
 * of tracyhip_alignment_rows are taken as they stand.  Rows may hold any byte; only '-' is a gap.  The two names are the caller's text,
 * printed byte for byte (never escaped, as the writers do not escape):
 *   PLOT   name0 = the first header line without its newline (">Alt", ">Alt1 (Estimated allelic Fraction: 0.5)": the double stays the
 *          caller's), name1 = the second (">Ref chr:a-b forward", ...).  Everything else is the device's: the two ungapped rows broken
 *          every linelimit + 14 letters, the score line, the rules, one block per linelimit columns with its two counters (the row-1
 *          counter runs upward from ref_pos + 1; forward == 0 and key != 3 prints ref_pos + ref_len - (letters of row 1 in front)), the
 *          spacer of 4 x (6 - blocks) newlines, the tail.  key: 0 .. 2 label "Alt" / "Ref" at setw(10), 3 "Alt1" / "Alt2" at setw(9).
 *   FASTA  ">" name0 "\n" row0 "\n>" name1 " (forward)" | " (reverse)" "\n" row1 "\n"  (name0 the trace stem, name1 rs.chr)
 *   JSON   from the ",\n\"refchr\": \"" behind assemblyTrace's closing brace through "\"forward\": 0|1\n}\n"; name1 = rs.chr (name0 is
 *          not read), refpos = ref_pos + 1.
 * The device answers an alignment when cols <= 2^22, both names are at most 65535 bytes, ref_pos >= 0 and
 * ref_pos + max(ref_len, cols) + 1 < 2^31, and -- PLOT with forward == 0 and key != 3 -- row 1 holds at most ref_len letters (found from
 * the data).  Any other alignment is DEFERRED: status and text_len = 0 are written, nothing else; tracyhost_alntext_batch prints it. */
#define TRACYHIP_ALNTEXT_PLOT  0
#define TRACYHIP_ALNTEXT_FASTA 1
#define TRACYHIP_ALNTEXT_JSON  2
#define TRACYHIP_ALNTEXT_OK 0
#define TRACYHIP_ALNTEXT_DEFERRED 1
#define TRACYHIP_ALNTEXT_TOO_SMALL 2 /* text_cap is too small: text_len is reported, no text is written */
typedef struct {
  uint32_t n, form;
  uint32_t key;                /* PLOT only: 0 .. 3 */
  uint32_t linelimit;          /* PLOT only: 1 .. 65535 */
  const uint8_t *rows0, *rows1; /* payload */
  const uint64_t* rows_offset; /* HOST array */
  const uint32_t* cols;        /* HOST array */
  const uint8_t* names;        /* payload: name0 of alignment i is name0_len[i] bytes at name0_offset[i], name1 likewise */
  const uint64_t* name0_offset; /* HOST arrays */
  const uint32_t* name0_len;
  const uint64_t* name1_offset;
  const uint32_t* name1_len;
  const int32_t* ref_pos;      /* HOST array: rs.pos */
  const uint32_t* ref_len;     /* HOST array: rs.refslice.size() */
  const uint8_t* forward;      /* HOST array: rs.forward */
  const int32_t* score;        /* HOST array (PLOT) */
} tracyhip_alntext_job;
typedef tracyhip_render_result tracyhip_alntext_result; /* status (TRACYHIP_ALNTEXT_*), text_len, text, text_offset, text_cap */
/* what tracyhip_render_alignments refuses before it touches a device (none is needed here): NULL job / result / required arrays, mem, form,
 * a PLOT with key > 3 or linelimit outside 1 .. 65535, a text without its offsets and capacities.  TRACYHIP_ERR_ARG (with the reason)
 * otherwise TRACYHIP_OK. */
int tracyhip_render_alignments_validate(const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out);
/* Three launches (count the bytes of every tile, scan them per alignment, emit) behind one that counts the letters of a plot's rows per
 * tile of columns; all but the last in the sizes-only form (text NULL).  Device payloads: ONE host synchronisation per call.  Host payloads are staged in chunks of consecutive
 * alignments within the workspace limit, with a second synchronisation each for the copy back of exactly the bytes that were reported.
 * An offset + length that leaves 64 bits is TRACYHIP_ERR_RANGE before any launch. */
int tracyhip_render_alignments(tracyhip_ctx* ctx, const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out);
/* an upper bound of text_len of an alignment of these sizes, whatever its bytes and numbers; needs no device.  0: no such form, or a
 * linelimit outside 1 .. 65535 for a PLOT. */
uint64_t tracyhip_render_alignments_bound(uint32_t form, uint32_t linelimit, uint32_t cols, uint32_t name0_len, uint32_t name1_len);
/* counters of the last tracyhip_render_alignments call of a context */
typedef struct {
  uint32_t alntext_chunks;    /* chunks of alignments the batch was cut into */
  uint32_t alntext_deferred;  /* alignments with TRACYHIP_ALNTEXT_DEFERRED */
  uint32_t alntext_too_small; /* alignments with TRACYHIP_ALNTEXT_TOO_SMALL */
} tracyhip_alntext_stats;
int tracyhip_last_alntext_stats(tracyhip_ctx* ctx, tracyhip_alntext_stats* out);

/* ---- the text `tracy decompose` prints from the decompose results themselves, byte for byte (tracy_amd/host indigo_out.hpp
 * writeDecomposition, traceAlleleAlignJsonTail, vcfRecordLines) -- where tracyhip_render_traces' JSON form and tracyhip_render_alignments
 * with key 3 stop -------------------------------------------------------------------------------------------------------------
 * The results are read where they lie: dcp_indel / dcp_err / dcp_offset of tracyhip_decompose_result, rows0 / rows1 of
 * tracyhip_alignment_rows for the three allele alignments, bcpos / estqual of the basecalls and the four arrays of
 * tracyhip_variants_result are taken as they stand.
 *   DECOMP  "indel\tdecomp\n", then one line indel "\t" err "\n" per table row (reads the table alone).
 *   JSON    from the ",\n\"chartConfig\": " behind the trace body through the final "}\n}\n": the viewport of the breakpoint, both allele
 *           blocks, the fractions, the alt-vs-alt rows, hetindel, the decomposition arrays, the variant rows and their x ranges.
 *   VCF     one record line per variant (no header: the date and the contig list are the caller's).  qual is 0 when the alt holds n / N;
 *           the GQ field carries estQual all the same.  Reads the basecalls, the variants and chr1.
 * Names are the caller's bytes, printed as they are (never escaped): chr1 / chr2 (rs.chr of the two alleles; v.chr of every variant
 * is chr1) and the two allelic fractions as the caller has printed them -- no floating-point number is formatted here.  v.id is ".".
 * trim_left / trim_right and qual_cut are truncated to 16 bits, as the writers' configuration holds them.  Computed here:
 * xWindowViewport of the breakpoint and of every variant, variantCallIndex from basenum (the records' call_index is not read),
 * variantType, the genotype words, LowQual / PASS, basepos, bcPos[q] + 1, every separator and the forms of empty lists.
 * A trace whose var_flags bit 0 is set, or whose decompose status is not 0, is the caller's to leave out of the batch: neither is
 * read here.  A dcp_rows, cols or var_n of 0 is legal and prints the empty forms.
 * DEFERRED (status and text_len = 0 are written, nothing else) -- JSON and VCF: a chr name longer than 65535 bytes (JSON: a fraction
 * too), bc_len = 0 (or beyond 2^31 - 1), var_n > max_variants, a variant whose call index is at or beyond bc_len (the host writer indexes unchecked) or
 * whose ref or alt range leaves its text region; JSON alone: trim_left + breakpoint at or beyond bc_len, cols > 2^22. */
#define TRACYHIP_DCPTEXT_DECOMP 0
#define TRACYHIP_DCPTEXT_JSON   1
#define TRACYHIP_DCPTEXT_VCF    2
#define TRACYHIP_DCPTEXT_OK 0
#define TRACYHIP_DCPTEXT_DEFERRED 1
#define TRACYHIP_DCPTEXT_TOO_SMALL 2 /* text_cap is too small: text_len is reported, no text is written */
typedef struct {
  uint32_t n, form;
  uint32_t qual_cut;              /* JSON, VCF */
  const int32_t *dcp_indel, *dcp_err; /* payload (DECOMP, JSON): trace t owns dcp_rows[t] entries from dcp_offset[t] on */
  const uint64_t* dcp_offset;     /* HOST array */
  const uint32_t* dcp_rows;       /* HOST array: rows of the table (tracyhip_decomp_status::dcp_n), at most 2^22 */
  const uint8_t* rows0[3];        /* payload (JSON): allele alignment k = 0, 1, 2 of trace t owns cols[k][t] bytes of rows0[k] and */
  const uint8_t* rows1[3];        /* of rows1[k] from rows_offset[k][t] on */
  const uint64_t* rows_offset[3]; /* HOST arrays */
  const uint32_t* cols[3];        /* HOST arrays */
  const int32_t* bcpos;           /* payload (JSON, VCF): trace t owns bc_len[t] entries from bc_offset[t] on, here and in estqual */
  const uint8_t* estqual;
  const uint64_t* bc_offset;      /* HOST array */
  const uint32_t* bc_len;         /* HOST array */
  const tracyhip_variant* var;    /* payload (JSON, VCF): as tracyhip_variants_result holds them */
  const uint8_t* var_text;
  const uint32_t* var_n;
  uint32_t max_variants;          /* 1 .. 1024 */
  uint32_t max_text;              /* 2 .. 2^19 */
  const uint32_t* var_index;      /* HOST array or NULL: the place of trace t in var (x max_variants), var_text (x max_text) and var_n; NULL: t.
                                     A batch that leaves traces of the variants call out says here where the others lie. */
  const uint32_t* ref_pos[2];     /* HOST arrays (JSON): rs.pos of the two alleles; ref1pos / ref2pos print it + 1 */
  const uint8_t* forward;         /* HOST array (JSON, VCF): rs.forward */
  const int32_t* score[3];        /* HOST arrays (JSON) */
  const uint32_t* breakpoint;     /* HOST array (JSON): bp.breakpoint as the report holds it */
  const uint8_t* indelshift;      /* HOST array (JSON) */
  const uint32_t *trim_left, *trim_right; /* HOST arrays (JSON, VCF), per trace */
  const uint8_t* names;           /* payload (JSON, VCF) */
  const uint64_t* chr_offset[2];  /* HOST arrays: chr1 (JSON, VCF), chr2 (JSON) */
  const uint32_t* chr_len[2];
  const uint64_t* frac_offset[2]; /* HOST arrays (JSON): the printed allele1fraction / allele2fraction */
  const uint32_t* frac_len[2];
} tracyhip_dcptext_job;
typedef tracyhip_render_result tracyhip_dcptext_result; /* status (TRACYHIP_DCPTEXT_*), text_len, text, text_offset, text_cap */
/* what tracyhip_render_decompositions refuses before it touches a device (none is needed here): NULL job / result / arrays its form reads,
 * mem, form, misaligned dcp_indel / dcp_err / bcpos / var / var_n, a text without its offsets and capacities (TRACYHIP_ERR_ARG);
 * max_variants outside 1 .. 1024, max_text outside 2 .. 2^19, a table of more than 2^22 rows (TRACYHIP_ERR_RANGE). */
int tracyhip_render_decompositions_validate(const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out);
/* Three launches (count the bytes of every tile, scan them per trace, emit); the first two alone in the sizes-only form (text NULL).
 * Device payloads: ONE host synchronisation per call.  Host payloads are staged in chunks of consecutive traces within the workspace
 * limit, with a second synchronisation each for the copy back of exactly the bytes that were reported.  The text does not depend on
 * the limit.  An offset + length that leaves 64 bits is TRACYHIP_ERR_RANGE before any launch. */
int tracyhip_render_decompositions(tracyhip_ctx* ctx, const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out);
/* the sizes a bound depends on; fields a form does not read are ignored */
typedef struct {
  uint32_t dcp_rows, cols[3], chr_len[2], frac_len[2], max_variants, max_text;
} tracyhip_dcptext_shape;
/* an upper bound of text_len of a trace of these sizes, whatever its bytes and numbers; needs no device.  0: no such form. */
uint64_t tracyhip_render_decompositions_bound(uint32_t form, const tracyhip_dcptext_shape* shape);
/* counters of the last tracyhip_render_decompositions call of a context */
typedef struct {
  uint32_t dcptext_chunks;    /* chunks of traces the batch was cut into */
  uint32_t dcptext_deferred;  /* traces with TRACYHIP_DCPTEXT_DEFERRED */
  uint32_t dcptext_too_small; /* traces with TRACYHIP_DCPTEXT_TOO_SMALL */
} tracyhip_dcptext_stats;
int tracyhip_last_dcptext_stats(tracyhip_ctx* ctx, tracyhip_dcptext_stats* out);

/* ---- the oriented reference slice of a CHAR-reference align job on the device: what the caller of tracyhip_align_traces does on the
 * host today between that call and tracyhip_alignment_rows ----------------------------------------------------------------------
 * Slice i = oriented.substr(slice_begin[i], slice_len[i]) at out + out_offset[i], where oriented is refs[ref_index ? ref_index[i] : i]
 * itself when forward[i] != 0 and otherwise its reverse complement by the byte rule of reverseComplement (fmindex.h:11-25: A C G T N in
 * either case complement to upper case; at any other letter the output position keeps the byte the reference has THERE).  forward,
 * slice_begin and slice_len are the arrays tracyhip_align_traces returned.  refs (kind CHAR) and out lie where `mem` says; the index and
 * offset arrays are HOST arrays.  Checked on the host before any launch: NULL arrays, refs of another kind, a ref_index out of range
 * (TRACYHIP_ERR_ARG); slice_begin + slice_len beyond the reference (TRACYHIP_ERR_RANGE).  One launch, one wave per tile of output bytes;
 * one host synchronisation.  The chain align_traces(MEM_DEVICE) -> reference_slices -> alignment_rows(MEM_DEVICE) ->
 * pad_traces / render_alignments then needs no payload on the host. */
typedef struct {
  uint32_t n;
  tracyhip_seqset refs;        /* kind CHAR */
  const uint32_t* ref_index;   /* HOST array or NULL (= identity) */
  const uint8_t* forward;      /* HOST arrays [n] */
  const uint32_t* slice_begin;
  const uint32_t* slice_len;
} tracyhip_slices_job;
int tracyhip_reference_slices_validate(const tracyhip_slices_job* job, int mem, const uint8_t* out, const uint64_t* out_offset);
int tracyhip_reference_slices(tracyhip_ctx* ctx, const tracyhip_slices_job* job, int mem, uint8_t* out, const uint64_t* out_offset);

/* ---- chromatogram files: a batch of ABIF / SCF file images turned into the arrays the readers produce (readab abif.h:286-405, traceFormat
 * scf.h:18-34, readscf scf.h:38-102) -- the first step of every command ----------------------------------------------------------
 * The images lie one after another in `bytes`, file t at file_offset[t] (any alignment), file_len[t] bytes long.  Every field of an
 * answered trace equals tracy_amd/host/trace_io.hpp (readab / readscf) for the same bytes: the four channels as A, C, G, T (ABIF: channel
 * i of DATA.9-12 is the letter FWO_.1[i]; PLOC and DATA are big-endian int16, sign-extended; SCF: second differences integrated twice
 * with a 16-bit carry), the call positions, basecalls1 / basecalls2 (letters other than ACGT become 'N'; NULs when P2BA is absent) and
 * qual (the PCON bytes), cut to the common length n = min(|PBAS|, |P2BA| unless absent, |PCON|, |PLOC|) where the character payloads are
 * taken one byte past their declared length, clipped at the end of the file.  For SCF basecalls1, basecalls2 and qual are zeros.
 * The device answers an ABIF file when the header and every directory slot (28 bytes each) lie inside the file, each of the nine keys
 * readab uses occurs at most once under the element type it is read under, with its natural element size and its payload inside the
 * file (in the slot itself iff the slot's dsize is <= 4), FWO_.1 starts with a permutation of ACGT, DATA.9-12 are all present with one
 * common count in 3 .. 2^23 that the file has room for (8 bytes a sample) and n is in 1 .. 131071; an SCF file when its version bytes
 * are [3-9].[0-9][0-9], samples is in 3 .. 2^23, bases in 1 .. 131071, both blocks lie inside the file and, with sample_bytes 2, every
 * integrated sample fits int16.  Any other file is DEFERRED: status and format are written, the sizes are zero, no payload is promised,
 * and the caller runs the host reader (the convention of tracyhip_basecall_traces). */
#define TRACYHIP_READ_OK 0
#define TRACYHIP_READ_DEFERRED 1
#define TRACYHIP_READ_TOO_SMALL 2 /* a capacity is too small: the sizes are reported, no payload is written */
typedef struct {
  uint32_t ntraces;
  const uint8_t* bytes;          /* payload: the file images */
  const uint64_t* file_offset;   /* HOST array, bytes, any alignment */
  const uint32_t* file_len;      /* HOST array */
  uint32_t sample_bytes;         /* 2 or 4: the width of the result signal */
} tracyhip_read_job;
/* The four per-trace arrays are HOST [ntraces] and required.  The payload results live where `mem` says and each may be NULL; with all of
 * them NULL the call is the sizes-only form, which needs no offsets or capacities.  With TRACYHIP_MEM_DEVICE the results are the inputs of
 * tracyhip_basecall_job as they stand: signal, signal_offset = sample_offset, nsamples, basecallpos, pos_offset = call_offset, npos =
 * ncalls. */
typedef struct {
  int32_t* status;         /* TRACYHIP_READ_* */
  int32_t* format;         /* 0 ABIF, 1 SCF, -1 neither, as traceFormat returns */
  uint32_t* nsamples;      /* samples per channel */
  uint32_t* ncalls;        /* the common length of positions, letters and qualities */
  void* signal;            /* sample_bytes as the job; trace t: channel k (A, C, G, T) at sample_offset[t] + k * nsamples[t] */
  const uint64_t* sample_offset; /* HOST array, elements */
  const uint32_t* sample_cap;    /* HOST array: samples per channel that trace t may take (4 * sample_cap[t] elements are its region) */
  int32_t* basecallpos;    /* ncalls[t] entries from call_offset[t] on, here and in the three below */
  uint8_t *basecalls1, *basecalls2, *qual;
  const uint64_t* call_offset;   /* HOST array */
  const uint32_t* call_cap;      /* HOST array */
} tracyhip_read_result;
/* what tracyhip_read_traces refuses before it touches a device (none is needed here): NULL job / result / required arrays, mem,
 * sample_bytes other than 2 or 4, a misaligned signal / basecallpos, a payload result without its offsets and capacities.
 * TRACYHIP_ERR_ARG (with the reason) otherwise TRACYHIP_OK. */
int tracyhip_read_validate(const tracyhip_read_job* job, int mem, const tracyhip_read_result* out);
/* capacities that any answered file of file_len bytes fits (four channels take at least 8 * nsamples bytes of the file, the positions at
 * least 2 * ncalls): with them a caller makes one call without the sizes-only pass.  Needs no device. */
int tracyhip_read_bound(uint32_t file_len, uint32_t* nsamples_max, uint32_t* ncalls_max);
/* Two launches: one wave per file scans header and directory (the sizes-only form ends here), one wave per (file, tile) writes the
 * payloads.  Device payloads: ONE host synchronisation per call.  Host payloads are staged in chunks of consecutive files within the
 * workspace limit (tracyhip_set_workspace_limit; 256 MB without one), with a second synchronisation each for the copy back of exactly what
 * was reported.  A file whose file_offset + file_len (or a result offset + capacity) leaves 64 bits is refused with TRACYHIP_ERR_RANGE
 * before the first launch. */
int tracyhip_read_traces(tracyhip_ctx* ctx, const tracyhip_read_job* job, int mem, const tracyhip_read_result* out);
/* counters of the last tracyhip_read_traces call of a context.  (A struct of their own: the layout of tracyhip_call_stats is pinned.) */
typedef struct {
  uint32_t read_chunks;    /* chunks of files the batch was cut into */
  uint32_t read_deferred;  /* traces with TRACYHIP_READ_DEFERRED */
  uint32_t read_too_small; /* traces with TRACYHIP_READ_TOO_SMALL */
} tracyhip_read_stats;
int tracyhip_last_read_stats(tracyhip_ctx* ctx, tracyhip_read_stats* out);

/* ---- reference-guided assembly (`tracy assemble -r`, assemble.h:219-288) for a batch of trace groups --------------------------
 * Group g owns the traces group_first[g] .. group_first[g + 1] - 1 (K of them) and the reference references[ref_index[g]].  Per group:
 *   1. the reverse complement of every trace (profile.h:74-90) and gotohScore(trace, reference), gotohScore(revcomp, reference)
 *      (assemble.h:219-226): gsFwd / gsRev -- one score launch for the whole batch
 *   2. a trace matches when gsFwd > thr || gsRev > thr with thr = len * match_fraction * match + len * (1 - match_fraction) * mismatch
 *      (len as double, the float terms promoted as assemble.h:229-230 writes them); it is forward iff gsFwd >= gsRev (:234); the matching
 *      traces are ordered by TraceScore (assemble.h:32-41): score descending, then input index
 *   3. gotoh(best, reference) (:250-252): the rows {_profileConsChar(best), _profileConsChar(reference)} along the alignment
 *   4. per further trace, best first (:253-284): _createProfile of the rows so far (align.h:138-180), gotoh(trace, that profile), the
 *      trace becomes row 0 and the old rows gain '-' where the alignment has a gap on their side (assemble.h:266-284)
 *   5. consensus() (msa.h:165-254) over all rows, the reference row left out unless include_reference (assemble.h:286-288)
 * Step k of all groups of a chunk is one batch of launches; the host reads the column counts once per step (they size the next
 * step's dynamic programs).  Rows, profiles and consensus equal the host chain's (tracy_amd/host/msa.hpp) bit for bit.
 * prm: any scoring tracyhip_gotoh_align accepts; the command uses {match, mismatch, go, ge, 1, 0} (AlignConfig<true,false>). */
typedef struct {
  uint32_t ngroups;
  tracyhip_seqset traces;        /* kind PROFILE: the trimmed FORWARD profile of every trace (createProfile(tr, bc, ., trimLeft, trimRight),
                                    assemble.h:199-217), every length >= 1, count >= group_first[ngroups] */
  const uint32_t* group_first;   /* HOST array [ngroups + 1], non-decreasing */
  tracyhip_seqset references;    /* kind PROFILE: _createProfile(reference slice), the `prefslice` of assemble.h:221, every used length >= 1 */
  const uint32_t* ref_index;     /* HOST array [ngroups], or NULL: group g uses reference g */
  float match_fraction;          /* matchFraction (-f, default 0.5) */
  float fraction_called;         /* fractionCalled (-d, default 0.1): covThreshold = (int32_t)(fraction_called * (float)rows), msa.h:196 */
  uint32_t include_reference;    /* incRef (-j): the reference row takes part in the consensus */
} tracyhip_assemble_job;

/* Result arrays where `mem` says; rows_offset / col_offset are HOST arrays.  With K traces in group g, n_ref reference columns and
 * sum_len the sum of the group's trace lengths, the caller provides
 *     (K + 1) * (n_ref + sum_len) bytes of `rows` from rows_offset[g] on, and
 *     n_ref + sum_len elements of gapped / cons / qual from col_offset[g] on
 * (an alignment of the chain never has more columns than n_ref + sum_len: every step adds at most its trace's length). */
typedef struct {
  int32_t* score_fwd;        /* [group_first[ngroups]], indexed like the traces set: gsFwd */
  int32_t* score_rev;        /* ... gsRev */
  uint8_t* forward;          /* ... 1 = gsFwd >= gsRev */
  uint32_t* rank;            /* ... position among the group's matching traces in TraceScore order; UINT32_MAX: excluded */
  uint32_t* nrows;           /* [ngroups] matching traces + 1; 0: none matches -- ncol and cons_len are 0 and no payload is written */
  uint32_t* ncol;            /* [ngroups] alignment columns */
  uint8_t* rows;             /* nrows x ncol bytes, packed, at rows_offset[g]: the trace of rank i is row nrows - 2 - i, the reference the last
                                (the order assemble.h:294-306 prints from) */
  uint8_t* gapped;           /* ncol bytes at col_offset[g]: the gapped consensus */
  uint8_t* cons;             /* cons_len bytes at col_offset[g]: its letters */
  uint8_t* qual;             /* cons_len bytes at col_offset[g]: their qualities as FASTQ characters (47 + maxCount * 10 / rows) */
  uint32_t* cons_len;        /* [ngroups] */
  const uint64_t* rows_offset;  /* HOST array [ngroups] */
  const uint64_t* col_offset;   /* HOST array [ngroups] */
} tracyhip_assemble_result;

/* what tracyhip_assemble_traces checks before it touches a device (none is needed here): NULL job / params / result / required arrays,
 * mem, sets that are not PROFILE, a group_first that decreases or runs past traces.count, a trace or used reference without columns,
 * a ref_index out of range, a match_fraction or fraction_called that is not a number.  TRACYHIP_ERR_ARG (with the reason) otherwise
 * TRACYHIP_OK. */
int tracyhip_assemble_validate(const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem, const tracyhip_assemble_result* out);
/* Host synchronisations: one for the profile classes, one for the strand scores, one per chain step of a chunk, one at the end
 * (tracyhip_call_stats::host_syncs; asm_chunks, asm_steps). */
int tracyhip_assemble_traces(tracyhip_ctx* ctx, const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem,
                             const tracyhip_assemble_result* out);

/* ---- de novo assembly (`tracy assemble` without -r, assemble.h:378-471 -> msa.h) for a batch of trace groups ---------------------
 * Group g owns the traces group_first[g] .. group_first[g + 1] - 1 (K of them).  Per group:
 *   1. the reverse complement of every trace (profile.h:74-90) and the strand table
 *          T[i][j][oi][oj] = gotohScore(strand oi of trace i as a1, strand oj of trace j as a2)
 *      for every ordered pair i != j and all four strand combinations: 4 K (K - 1) pairs, ONE family of score launches for the
 *      whole batch.  (No entry follows from another: the 25-term fp32 sum changes its order under reverse complement and under
 *      swapping the sides.)  The sequential loop of the reference scores K (K - 1) / 2 + iterations * K (K - 1) pairs, with at least
 *      two iterations on any input with a positive score: the table is at most about 1.6 x those cells, removes iterations * K
 *      dependent launches and supplies every score of steps 3 and 4.
 *   2. revSeqBasedOnDist (msa.h:258-323) on the host, from the table: one strand bit per trace (a double flip is the original
 *      profile bit for bit)
 *   3. the overlap test of assemble.h:425-456, in rounds: every undecided trace i aligns with its next partner j (gotoh with
 *      traceback), numAligned = the 's' ops, gs = T[i][j][o_i][o_j]; the trace stays when
 *          numAligned / len_i > 0.1 && numAligned > 25 && gs > numAligned * match_fraction * match + numAligned * (1 - match_fraction) * mismatch
 *      (int x float products, a float sum, then promoted: assemble.h:441); a trace that runs out of partners is excluded
 *   4. msa() (msa.h:326-368) of the traces that stay, when there are at least two: the distance matrix comes from the table, UPGMA
 *      and the node heights run on the host, the merges of one height are one batch -- gotoh(left, right), the rows of the left
 *      child above those of the right one (msa.h:121-150), _createProfile (align.h:138-180) of every node below the root
 *   5. consensus() (msa.h:165-254) over all rows
 * Rows, profiles and consensus equal the per-group host path's (tracy_amd/host/msa.hpp) bit for bit.
 * prm: any scoring tracyhip_gotoh_align accepts; the command uses {match, mismatch, go, ge, 1, 1} (AlignConfig<true,true>). */
typedef struct {
  uint32_t ngroups;
  tracyhip_seqset traces;        /* kind PROFILE: the trimmed FORWARD profile of every trace (assemble.h:384-417), every length >= 1,
                                    count >= group_first[ngroups] */
  const uint32_t* group_first;   /* HOST array [ngroups + 1], non-decreasing */
  float match_fraction;          /* matchFraction (-f, default 0.5) */
  float fraction_called;         /* fractionCalled (-d, default 0.1): covThreshold = (int32_t)(fraction_called * (float)rows), msa.h:196 */
} tracyhip_denovo_job;

/* Result arrays where `mem` says; rows_offset / col_offset are HOST arrays.  With K traces in group g and sum_len the sum of their
 * lengths the caller provides
 *     K * sum_len bytes of `rows` from rows_offset[g] on, and
 *     sum_len elements of gapped / cons / qual from col_offset[g] on
 * (every merge adds at most the columns of its two sides). */
typedef struct {
  uint8_t* forward;          /* [group_first[ngroups]], indexed like the traces set: fwdProfiles[i] after revSeqBasedOnDist */
  uint32_t* partner;         /* ... the index within the group of the first j that passed the overlap test; UINT32_MAX: excluded */
  uint32_t* row;             /* ... the trace's row in the group's alignment; UINT32_MAX: none (excluded -- or UPGMA stopped on negative
                                scores before the trace was joined, msa.h:86: the alignment is then the last node made) */
  uint32_t* nrows;           /* [ngroups] 0: fewer than two traces stay ("At least 2 traces are required") -- ncol and cons_len are 0 and
                                no payload is written */
  uint32_t* ncol;            /* [ngroups] alignment columns */
  uint8_t* rows;             /* nrows x ncol bytes, packed, at rows_offset[g], in the order msa() returns them */
  uint8_t* gapped;           /* as tracyhip_assemble_result */
  uint8_t* cons;
  uint8_t* qual;
  uint32_t* cons_len;        /* [ngroups] */
  const uint64_t* rows_offset;  /* HOST array [ngroups] */
  const uint64_t* col_offset;   /* HOST array [ngroups] */
} tracyhip_denovo_result;

/* what tracyhip_denovo_traces checks before it touches a device (none is needed here): what tracyhip_assemble_validate checks,
 * without the references.  An empty batch, a group without traces and a group of one trace are fine (nrows 0). */
int tracyhip_denovo_validate(const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem, const tracyhip_denovo_result* out);
/* The batch is cut into chunks of groups whose traceback planes fit the workspace limit (tracyhip_set_workspace_limit); a chunk runs
 * its overlap rounds, then its tree heights, then its consensus.  Host synchronisations (tracyhip_call_stats::host_syncs):
 *     1 (profile classes) + 1 (strand table) + denovo_rounds + denovo_steps + 1 (the end)
 * where a chunk adds to denovo_rounds the largest number of partners any of its traces tries and to denovo_steps the height of its
 * tallest tree -- neither depends on how many groups the chunk holds.  Un-normalised profiles that leave the 16-bit score range
 * repeat the call on int32 after the table: 2 more. */
int tracyhip_denovo_traces(tracyhip_ctx* ctx, const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem,
                           const tracyhip_denovo_result* out);

/* ---- device memory for a caller without a HIP runtime of its own (the command line): buffers for the payloads of the calls that take
 * TRACYHIP_MEM_DEVICE, so that a chain of them (tracyhip_read_traces -> tracyhip_basecall_traces -> tracyhip_render_traces) keeps every
 * intermediate on the device.  tracyhip_device_copy is synchronous on the context's stream: it runs behind the calls issued before it
 * and has finished when it returns (to_device != 0: host -> device, else device -> host). */
int tracyhip_device_alloc(tracyhip_ctx* ctx, uint64_t bytes, void** out);
int tracyhip_device_free(tracyhip_ctx* ctx, void* p);
int tracyhip_device_copy(tracyhip_ctx* ctx, void* dst, const void* src, uint64_t bytes, int to_device);

/* ---- asynchronous forms (SURVEY.md 8b "Threading": synchronous by default with an async variant) ---------------------
 * Same arguments and results as the call without the suffix; the call returns as soon as the work is queued on the
 * context.  A context executes its calls in issue order on its own worker thread and stream (the pipelines need the
 * host between kernels -- orientation decision, trimReferenceSlice geometry -- so "enqueue" means this queue, not only
 * the HIP stream).  The structs are copied; every array they point to (inputs, offsets, results) must stay valid and
 * untouched until tracyhip_synchronize(ctx) returns, which is also when results are final and errors are reported.
 * A synchronous call on a context with queued work waits for that work first.  Several contexts (one per host thread,
 * or the members of a group) run concurrently. */
int tracyhip_gotoh_score_async(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, const tracyhip_params* prm, int mem, int32_t* scores);
int tracyhip_gotoh_align_async(tracyhip_ctx* ctx, const tracyhip_pairs* pairs, const tracyhip_params* prm, int mem, int32_t* scores,
                               uint8_t* ops, const uint64_t* ops_offset, uint32_t* ops_len);
int tracyhip_align_traces_async(tracyhip_ctx* ctx, const tracyhip_align_job* job, const tracyhip_params* prm, int mem,
                                const tracyhip_align_result* out);
int tracyhip_decompose_traces_async(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_params* prm, int mem,
                                    const tracyhip_decompose_result* out);
int tracyhip_consensus_traces_async(tracyhip_ctx* ctx, const tracyhip_consensus_job* job, const tracyhip_params* prm, int mem,
                                    const tracyhip_consensus_result* out);
int tracyhip_basecall_traces_async(tracyhip_ctx* ctx, const tracyhip_basecall_job* job, int mem, const tracyhip_basecall_result* out);
int tracyhip_pad_traces_async(tracyhip_ctx* ctx, const tracyhip_pad_job* job, int mem, const tracyhip_pad_result* out);
int tracyhip_render_traces_async(tracyhip_ctx* ctx, const tracyhip_render_job* job, int mem, const tracyhip_render_result* out);
int tracyhip_read_traces_async(tracyhip_ctx* ctx, const tracyhip_read_job* job, int mem, const tracyhip_read_result* out);
int tracyhip_render_alignments_async(tracyhip_ctx* ctx, const tracyhip_alntext_job* job, int mem, const tracyhip_alntext_result* out);
int tracyhip_render_decompositions_async(tracyhip_ctx* ctx, const tracyhip_dcptext_job* job, int mem, const tracyhip_dcptext_result* out);
int tracyhip_reference_slices_async(tracyhip_ctx* ctx, const tracyhip_slices_job* job, int mem, uint8_t* out, const uint64_t* out_offset);
int tracyhip_assemble_traces_async(tracyhip_ctx* ctx, const tracyhip_assemble_job* job, const tracyhip_params* prm, int mem,
                                   const tracyhip_assemble_result* out);
int tracyhip_denovo_traces_async(tracyhip_ctx* ctx, const tracyhip_denovo_job* job, const tracyhip_params* prm, int mem,
                                 const tracyhip_denovo_result* out);
/* (slice_pos is copied too: it need not outlive the call) */
int tracyhip_decompose_variants_async(tracyhip_ctx* ctx, const tracyhip_decompose_job* job, const tracyhip_decompose_result* res,
                                      const uint32_t* slice_pos, const tracyhip_params* prm, int mem, const tracyhip_variants_result* out);

/* ---- device groups: the GPUs of one node behind one handle (north star: "batches of traces shard embarrassingly across
 * the 8 GPUs of one node") ------------------------------------------------------------------------------------------
 * One context per device, one host thread per context.  A batch call on a group cuts the batch into contiguous blocks
 * of traces (tracyhip_group_gotoh_score: the pair list into slices of equal DP cell count, the sequence sets replicated --
 * the all-pairs matrix of msa.h:33-42), runs each block through its device and returns when all are complete; results
 * land in the caller's arrays exactly as from the single-device call.  HOST buffers only (every block stages its own part
 * through its own device; nothing crosses devices).  devices == NULL: the first `ndevices` visible devices (0 = all).
 * A device may be listed more than once (two contexts on one GPU).  Multi-PROCESS jobs use one plain context per rank
 * and gather over RCCL instead (tracy_amd/shard.py, bench.py). */
typedef struct tracyhip_group tracyhip_group;
int tracyhip_group_create(const int* devices, int ndevices, tracyhip_group** group);
int tracyhip_group_destroy(tracyhip_group* group);
int tracyhip_group_size(const tracyhip_group* group);
tracyhip_ctx* tracyhip_group_context(tracyhip_group* group, int i); /* member i, e.g. for tracyhip_set_workspace_limit */
int tracyhip_group_set_lanes(tracyhip_group* group, uint32_t lanes);
int tracyhip_group_gotoh_score(tracyhip_group* group, const tracyhip_pairs* pairs, const tracyhip_params* prm, int32_t* scores);
int tracyhip_group_align_traces(tracyhip_group* group, const tracyhip_align_job* job, const tracyhip_params* prm,
                                const tracyhip_align_result* out);
int tracyhip_group_decompose_traces(tracyhip_group* group, const tracyhip_decompose_job* job, const tracyhip_params* prm,
                                    const tracyhip_decompose_result* out);
/* bounds[0 .. parts] of `parts` contiguous slices of the pair list with (nearly) equal DP cell count; host arithmetic, no device */
int tracyhip_pair_bounds(const tracyhip_pairs* pairs, uint32_t parts, uint64_t* bounds);

/* ---- result compaction for the final gather of a sharded job (no counterpart in the reference, which is one process) ----
 * The pipelines write variable-length results (traceback strings, decomposition tables) into fixed-capacity regions the caller lays out
 * (ops_offset[t] = t * capacity, dcp_offset[t] = t * (2 maxindel + 2)).  Before a rank ships them to the rank that collects the job's
 * results it packs the used parts back to back: region i of a payload kind = bytes [i * stride_bytes, (i + 1) * stride_bytes) of src, of
 * which the first lens[i * lens_stride] * elem_bytes bytes are used (never more than the stride).  src, lens and dst are DEVICE pointers;
 * lens_stride lets a field of a record array serve (tracyhip_decomp_status::dcp_n: lens = &dstatus[0].dcp_n, lens_stride = 6).
 * tracyhip_pack_ragged_multi packs up to 16 kinds in one pass, kind-major (all regions of kind 0 in region order, then kind 1, ...) --
 * one scan, one copy launch, one synchronisation; kind_bytes[k] (HOST) receives the packed size of kind k.  dst == NULL: sizes only.
 * TRACYHIP_ERR_ARG when the total exceeds dst_cap (nothing is written then; with dst_cap >= the sum of n * stride_bytes the copy is
 * queued without waiting for the sizes).  Synchronous. */
typedef struct {
  const void* src;
  uint64_t stride_bytes;
  uint32_t elem_bytes;
  const uint32_t* lens;
  uint32_t lens_stride;
} tracyhip_ragged_src;
int tracyhip_pack_ragged_multi(tracyhip_ctx* ctx, const tracyhip_ragged_src* kinds, uint32_t nkinds, uint32_t n, void* dst, uint64_t dst_cap,
                               uint64_t* kind_bytes);
int tracyhip_pack_ragged(tracyhip_ctx* ctx, const void* src, uint64_t stride_bytes, uint32_t elem_bytes, const uint32_t* lens, uint32_t lens_stride,
                         uint32_t n, void* dst, uint64_t dst_cap, uint64_t* total_bytes);

/* ---- kernel timing (HIP events recorded on the context's stream around each DP / walker launch) ---
 * The reference has only the optional gperftools wrapper (sage.h:60-62); this is the hook bench.py uses
 * for its roofline line.  bytes = ALGORITHMIC bytes of the launches: 0.5 B per traceback cell + the
 * inputs once (1 B per reference base, 24 B per profile column, 1 B per string base) + 4 B score. */
#define TRACYHIP_TIMER_SCORE 0 /* score-only DP kernels */
#define TRACYHIP_TIMER_TRACE 1 /* traceback DP kernels  */
#define TRACYHIP_TIMER_WALK 2  /* traceback walkers     */
#define TRACYHIP_TIMER_BAND 3  /* band tracebacks (checkpointed traceback of the align / decompose pipelines); cells = the cells the
                                  kernel really re-swept (strip height x steps of the bands its paths cross), not m x n */
#define TRACYHIP_TIMER_PREFIX 4 /* prefix-bound kernels (strand by certificate); cells = rows actually swept x columns */
#define TRACYHIP_TIMER_ORIGIN 5 /* origin-tracking sweeps (gotoh() whose alignment only trimReferenceSlice reads) */
#define TRACYHIP_TIMER_DECOMP 6 /* decomposeAlleles kernel; cells = alignment columns, bytes = rows + basecalls + table */
#define TRACYHIP_TIMER_AFRAC 7  /* allelicFraction kernel; cells = grid points x diffnuc bound, bytes = signal windows read */
#define TRACYHIP_TIMER_MISC 8   /* findBreakpoint, findHomozygousBreakpoint, generateSecondaryDecomposed, alignment rows, trims, trace padding */
#define TRACYHIP_TIMER_FRONT 9  /* pruned orientation sweep of `tracy align` (front.h): band placement, the band sweep below the prefix
                                   rows, certificate; cells = the band's, bytes = tables + codes + the kept row (read twice) */
#define TRACYHIP_TIMER_COUNT 10
typedef struct {
  double ms;         /* summed launch durations */
  uint64_t launches;
  uint64_t cells;    /* DP cells (m*n summed over pairs) */
  uint64_t bytes;    /* algorithmic HBM bytes */
} tracyhip_kernel_timing;
int tracyhip_timing_enable(tracyhip_ctx* ctx, int on);
int tracyhip_timing_reset(tracyhip_ctx* ctx);
int tracyhip_timing_get(tracyhip_ctx* ctx, int which, tracyhip_kernel_timing* out);

#ifdef __cplusplus
}
#endif
#endif
