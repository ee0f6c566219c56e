/*
 * deepgrp_hip.h -- C ABI of libdeepgrp_hip.so, the MI355X (gfx950) implementation of
 * DeepGRP's prediction hot path.
 *
 * This is the drop-in boundary: plain C, raw pointers and sizes, no torch / Python
 * types.  Every entry point names the reference interface it replaces (paths are
 * relative to the upstream fhausmann/deepgrp repository).  The reference has two C
 * symbols on this path (`_get_max`, deepgrp/maxcalc.h:3-4, and `mss_find_all`,
 * deepgrp/_mss/mss.h:16-17) and otherwise crosses into compiled code through Cython
 * (deepgrp/sequence.pyx, deepgrp/_mss/pymss.pyx) and TensorFlow
 * (`model.predict_on_batch`, deepgrp/prediction.py:106).  INTEGRATION.md shows the
 * ctypes stubs a maintainer would add on the reference side.
 *
 * Conventions
 *   - every function returns 0 on success and a negative DGRP_E* code on failure;
 *     dgrp_last_error() returns a thread-local message for the last failure;
 *   - pointers prefixed d_ are DEVICE pointers (HBM, allocated by the caller, e.g. by
 *     torch.empty(..., device="cuda")); h_ are host pointers;
 *   - `stream` is a hipStream_t passed as void* (NULL = the default stream); all work
 *     is enqueued asynchronously on it unless a function says it synchronises;
 *   - functions are re-entrant; a dgrp_model may be shared by threads that use
 *     different streams and workspaces.
 */
#ifndef DEEPGRP_HIP_H_
#define DEEPGRP_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define DGRP_OK 0
#define DGRP_EINVAL (-1)   /* bad argument (shape, NULL pointer, unsupported size)   */
#define DGRP_EHIP (-2)     /* a HIP runtime call or kernel launch failed              */
#define DGRP_ENOMEM (-3)   /* caller-provided workspace / output capacity too small   */
#define DGRP_ENODEV (-4)   /* no gfx950 device visible                                */
/* DGRP_EDATA (-5): corrupt compressed input, see dgrp_inflate_batch */

#define DGRP_ABI_VERSION 1

/* Segment record written by dgrp_segments(): one TSV row of deepgrp/__main__.py:288-292
 * without the two name columns. */
typedef struct dgrp_segment {
    int64_t start;   /* 0-based, inclusive, in ORIGINAL (unstripped) record coordinates */
    int64_t end;     /* exclusive                                                         */
    int32_t label;   /* 1..C-1                                                            */
    int32_t contig;  /* caller-defined tag copied from the call (record index)            */
} dgrp_segment;

typedef struct dgrp_model dgrp_model;   /* opaque: packed weights resident in HBM */

int dgrp_abi_version(void);
const char *dgrp_last_error(void);
/* Name / CU count / HBM bytes of the current device (synchronous). */
int dgrp_device_info(char *name, size_t name_cap, int *cu_count, int64_t *hbm_bytes);

/* ---- A2: deepgrp.sequence.one_hot_encode_dna_sequence (deepgrp/sequence.pyx:19-36, :55-58)
 * Host helper: number of leading exact 'N' bytes and kept length after dropping leading and
 * trailing 'N' (negative for an all-N record: the reference raises ValueError there). */
int dgrp_strip_n(const uint8_t *h_seq, int64_t len, int64_t *startpos, int64_t *kept);
/* bytes -> class index 0..4 per base (A,a=0 C,c=1 G,g=2 T,t=3 else 4), the compact form every
 * other kernel consumes. */
int dgrp_encode(const uint8_t *d_seq, int64_t n, uint8_t *d_idx, void *stream);
/* bytes -> int8 [5, n] C-order, exactly the array the reference function returns. */
int dgrp_onehot(const uint8_t *d_seq, int64_t n, int8_t *d_onehot, void *stream);

/* ---- A1+A2 fused for one record body: _read_multi_fasta's per-line strip()/upper()/join
 * (deepgrp/__main__.py:31-41) followed by one_hot_encode_dna_sequence's N stripping and class lookup
 * (deepgrp/sequence.pyx:27-35), on the raw bytes between a header line and the next header.
 * d_raw [nbytes] device bytes as they are in the file; d_idx receives one class index per sequence
 * character (line ends removed), BEFORE N stripping, capacity nbytes.  h_info (host, filled after a
 * stream synchronisation): [0] 1 if the body is "plain" (ASCII, no whitespace except LF / CRLF line
 * ends, no blank line) so that deleting line ends equals stripping every line -- otherwise the caller
 * must parse this record with the reference loop; [1] sequence length; [2] startpos = number of leading
 * 'N'/'n'; [3] kept length after dropping leading and trailing N (negative for an all-N record).
 * The class indices of the kept part are d_idx[startpos .. startpos + kept). */
int64_t dgrp_fasta_workspace_bytes(int64_t nbytes);
int dgrp_fasta_encode(const uint8_t *d_raw, int64_t nbytes, uint8_t *d_idx, int64_t *h_info, void *d_work,
                      int64_t work_bytes, void *stream);

/* The same for nrec record bodies of ONE device buffer in a single call (one read-back, one synchronisation):
 * record r = bytes [h_off[r], h_off[r] + h_len[r]) of d_raw, its indices go to d_idx + h_off[r], its four info
 * values to h_info[4 r ..].  For files of many short records. */
int64_t dgrp_fasta_batch_workspace_bytes(int64_t nrec, int64_t total_bytes);
int dgrp_fasta_encode_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                            uint8_t *d_idx, int64_t *h_info, void *d_work, int64_t work_bytes, void *stream);

/* ---- A1: where the records of an uploaded FASTA file start (_read_multi_fasta, deepgrp/__main__.py:31-41: a line whose first
 * character is '>' opens a record).  d_raw [nbytes] = the file as it is, 16-byte aligned.  A chunk starts at byte 0 and at every '>'
 * that directly follows a line feed.  h_start[0..n) ascending chunk starts, h_first_lf[i] = position of the first line feed in chunk i
 * (nbytes if it has none: the header line runs to the chunk's end).  *n_chunks = chunks found; if it exceeds cap nothing else is
 * valid: call again with cap >= *n_chunks.  Synchronous.  Replaces host passes over the file bytes (numpy compare + nonzero). */
int64_t dgrp_fasta_chunks_workspace_bytes(int64_t cap);
int dgrp_fasta_chunks(const uint8_t *d_raw, int64_t nbytes, int64_t cap, int64_t *h_start, int64_t *h_first_lf,
                      int64_t *n_chunks, void *d_work, int64_t work_bytes, void *stream);

/* ---- Masked FASTA (predict --mask_dir; an addition, no counterpart in the reference): the sequence bytes of nrec plain record
 * bodies of ONE device buffer rewritten after the TSV rows of their records.  Record r = bytes [h_off[r], h_off[r] + h_len[r]) of
 * d_raw, a body that dgrp_fasta_encode_batch calls plain (LF or CRLF line ends only); its sequence position p is the p-th byte that
 * is neither CR nor LF, the coordinate of the TSV rows.  Its rows are d_rows[h_row_off[r] .. h_row_off[r+1]) (device), ascending
 * and disjoint, 0 <= start < end <= its sequence length (else DGRP_EINVAL before anything is written).  A position is inside when a
 * row with (class_mask >> label) & 1 covers it.  mode 0 (soft): ASCII letters inside -> lower case, other letters -> upper case;
 * mode 1 (hard): inside -> 'N', other bytes unchanged.  Line ends are copied.  The bytes land at the same offsets of d_out (may be
 * d_raw); nothing else of d_out is written.  d_raw and d_out 16-byte aligned.  Stream-ordered after the row check (which
 * synchronises once). */
int64_t dgrp_fasta_mask_workspace_bytes(int64_t nrec, int64_t total_bytes, int64_t nrows);
int dgrp_fasta_mask_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                          const dgrp_segment *d_rows, const int64_t *h_row_off, int mode, uint64_t class_mask,
                          uint8_t *d_out, void *d_work, int64_t work_bytes, void *stream);

/* ---- UCSC .2bit input (an addition; the reference reads FASTA text only).  d_file [file_bytes] = the .2bit file as it is, any
 * alignment.  Record r has h_dna_size[r] bases (at most 2^32 - 1), packed four per byte from file offset h_packed_off[r]: T=0 C=1
 * A=2 G=3, the first base of a byte in its two most significant bits, the unused bits of the last byte arbitrary.  Its N blocks are
 * the intervals h_n_iv_off[r] .. h_n_iv_off[r + 1] of d_n_iv (device, n_iv intervals as int64 pairs [start, end)): ascending,
 * disjoint, inside the record (the host parser merges the file's blocks; an interval that is not only costs or loses N, no access
 * leaves a buffer).  Every host table is read before the call returns and checked against file_bytes, n_iv and the output
 * capacity (DGRP_EINVAL before anything is queued); the work is stream-ordered, nothing synchronises or reads back.
 * Workspace of either entry: dgrp_twobit_workspace_bytes of nrec (else DGRP_ENOMEM).  nrec == 0: nothing is queued.
 *
 * dgrp_twobit_encode_batch: one class index per base (A=0 C=1 G=2 T=3, inside an N block 4 whatever the two bits say -- what
 * dgrp_encode gives for the letters) to d_idx[h_out_off[r] .. + h_dna_size[r]), the WHOLE record before N stripping, as
 * dgrp_fasta_encode; nothing else of d_idx [idx_cap] is written.  Any alignment of packed bytes and output is correct; a lane
 * owns one 16-byte aligned word of d_idx and stores it whole where it lies inside the record.  With o = (d_idx + h_out_off[r]) mod
 * 16, word g of record r starts with base 16 g - o, i.e. with packed byte 4 g - o / 4 when o is a multiple of 4; the lane reads its
 * four packed bytes in one 4-byte load when that byte's address is a multiple of 4, which holds for every word of the record when
 * o = 4 * (address of the record's packed bytes mod 4) -- the caller chooses h_out_off so (twobit.placed_offsets) -- and in five
 * byte loads otherwise.
 *
 * dgrp_twobit_text_batch: the FASTA text of the records -- '>', the h_name_len[r] (<= 255) name bytes at file offset
 * h_name_off[r], LF, then the bases 50 per line, every line LF-terminated (no base: the header line only); letters ACGT, N inside
 * an N block, lower case inside a soft-mask interval (d_m_iv, h_m_iv_off, m_iv: as the N intervals) -- to d_text[h_text_off[r] ..
 * + 2 + h_name_len[r] + h_dna_size[r] + ceil(h_dna_size[r] / 50)); nothing else of d_text [text_cap] is written. */
int64_t dgrp_twobit_workspace_bytes(int64_t nrec);
int dgrp_twobit_encode_batch(const uint8_t *d_file, int64_t file_bytes, int64_t nrec, const int64_t *h_packed_off,
                             const int64_t *h_dna_size, const int64_t *d_n_iv, const int64_t *h_n_iv_off, int64_t n_iv,
                             const int64_t *h_out_off, uint8_t *d_idx, int64_t idx_cap, void *d_work, int64_t work_bytes,
                             void *stream);
int dgrp_twobit_text_batch(const uint8_t *d_file, int64_t file_bytes, int64_t nrec, const int64_t *h_name_off,
                           const int64_t *h_name_len, const int64_t *h_packed_off, const int64_t *h_dna_size,
                           const int64_t *d_n_iv, const int64_t *h_n_iv_off, int64_t n_iv, const int64_t *d_m_iv,
                           const int64_t *h_m_iv_off, int64_t m_iv, const int64_t *h_text_off, uint8_t *d_text,
                           int64_t text_cap, void *d_work, int64_t work_bytes, void *stream);

/* ---- UCSC .2bit output (predict --mask_twobit; an addition): the records of a 2bit file from nrec plain record bodies of ONE
 * device buffer, addressed as dgrp_fasta_mask_batch addresses them -- record r = bytes [h_off[r], h_off[r] + h_len[r]) of d_raw
 * (16-byte aligned), line ends LF or CRLF, sequence position p = the p-th byte that is neither CR nor LF, the last line with or
 * without its line end.  It runs on the bytes that dgrp_fasta_mask_batch has just rewritten.  Per sequence byte: A C G T in either
 * case pack to T=0 C=1 A=2 G=3, the first base of a byte in its two most significant bits, the unused bits of the last byte 0; any
 * other byte is N (two bits 0); a byte 'a'..'z' is soft-masked.  The N blocks and the mask blocks of a record are the maximal runs
 * of such bytes: ascending, disjoint, never adjacent, never empty.
 * Stage 1 counts per tile of text and scans (scan.h, three launches); per record dnaSize, nBlockCount and maskBlockCount come back
 * to h_counts[3 r ..] -- the entry's only synchronisation.  Stage 2: the blobs
 *     dnaSize, nBlockCount, nBlockStarts[], nBlockSizes[], maskBlockCount, maskBlockStarts[], maskBlockSizes[], reserved (0),
 *     packedDna (ceil(dnaSize / 4) bytes)
 * (uint32, little-endian) are laid out back to back from d_out + out_off, each at whatever byte alignment falls out, record r at
 * h_blob_off[r], the end of the last at h_blob_off[nrec]; the kernels write every blob whole and nothing else of d_out [out_cap].
 * Checked before anything is queued: the host tables (DGRP_EINVAL; at most 2^32 - 1 bytes of text per call), the workspace
 * (dgrp_twobit_pack_workspace_bytes, else DGRP_ENOMEM) and room for the 16 bytes every blob has (DGRP_ENOMEM).  Blobs that do not
 * fit out_cap once their sizes are known: DGRP_ENOMEM with h_counts and h_blob_off filled and nothing written -- call again with
 * h_blob_off[nrec] bytes.  nrec == 0: nothing is queued.  The writes are stream-ordered. */
int64_t dgrp_twobit_pack_workspace_bytes(int64_t nrec, int64_t total_bytes);
int dgrp_twobit_pack_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len, uint8_t *d_out,
                           int64_t out_off, int64_t out_cap, int64_t *h_counts, int64_t *h_blob_off, void *d_work,
                           int64_t work_bytes, void *stream);

/* ---- FASTA of the predicted repeats (predict --seq_dir; an addition): the sequence bytes under the TSV rows of nrec plain record
 * bodies of ONE device buffer, gathered into one compact text.  Records and rows are as for dgrp_fasta_mask_batch: record r = bytes
 * [h_off[r], h_off[r] + h_len[r]) of d_raw (16-byte aligned; the ranges ascend and do not overlap), a body with LF or CRLF line
 * ends, sequence position p = the p-th byte that is neither CR nor LF; its rows are d_rows[h_row_off[r] .. h_row_off[r + 1])
 * (device; any ascending sub-range of the record's rows), ascending and disjoint, 0 <= start < end <= its sequence length.  Its
 * name is the bytes d_names[h_name_off[r] .. h_name_off[r + 1]) (device, the names back to back, h_name_off [nrec + 1]; at most
 * 2^20 bytes a name).  A row is kept when (class_mask >> label) & 1.  For a kept row (start, end, label) of a record of len sequence
 * positions, with A = start - min(flank, start) and B = end + min(flank, len - end), the text is
 *     >NAME:A-B class<label>LF                      (flank == 0)
 *     >NAME:A-B class<label> core=<start>-<end>LF   (flank > 0)
 * followed by the bytes of the sequence positions [A, B) exactly as they are in d_raw, `width` (1 .. 2^30) per line, every line
 * LF-terminated; numbers are plain decimal.  Every row is read independently: flanks may overlap other rows.  The texts of the kept
 * rows are written back to back from d_text[0] in row order; *h_text_bytes is their exact size and *h_kept the number of kept rows;
 * with d_entries (may be NULL; room for one entry per row) entry k states where kept row k's header starts (text_off), where its
 * first base stands (base_off) and how many bases it has.  No byte of d_text at or beyond *h_text_bytes is ever written.
 * Checked first, before any device pointer is touched: the host tables and scalars (DGRP_EINVAL), then the workspace
 * (dgrp_fasta_extract_workspace_bytes of nrec, the sum of h_len and the number of rows; else DGRP_ENOMEM).  nrec == 0 or no rows at
 * all: nothing to do, both sizes 0.  A bad row: DGRP_EINVAL naming the row, nothing of d_text or d_entries written.  A text larger
 * than text_cap: DGRP_ENOMEM with *h_text_bytes (the size to call again with) and *h_kept set, nothing written.
 * Stages: sequence bytes per 4096-byte body tile and in front of every 16-byte word of a tile, scanned; one lane per row checks it
 * and states its text bytes, scanned; the sizes and the row check are read back -- the entry's one synchronisation of `stream`;
 * then one workgroup per 4096 bytes of text, 16 per lane: a lane finds its row by binary search over the scanned sizes, formats the
 * header bytes that fall to it, finds its first source byte by binary search over the record's tile prefix and the tile's word
 * counts and copies on from there, a line feed behind every `width`-th base.  The write is stream-ordered behind the read-back. */
typedef struct dgrp_extract_entry {
    int64_t text_off;   /* offset in d_text of the '>' of the row's header line */
    int64_t base_off;   /* offset in d_text of the row's first base             */
    int64_t bases;      /* B - A                                                */
} dgrp_extract_entry;
int64_t dgrp_fasta_extract_workspace_bytes(int64_t nrec, int64_t total_bytes, int64_t nrows);
int dgrp_fasta_extract_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                             const dgrp_segment *d_rows, const int64_t *h_row_off, const uint8_t *d_names,
                             const int64_t *h_name_off, int64_t flank, int width, uint64_t class_mask, uint8_t *d_text,
                             int64_t text_cap, int64_t *h_text_bytes, dgrp_extract_entry *d_entries, int64_t *h_kept,
                             void *d_work, int64_t work_bytes, void *stream);

/* ---- Repeat content table (predict --summary_dir; an addition): how much of every record lies under every label, by kind of byte
 * and case, and -- with bin > 0 -- per bin of `bin` sequence positions.  Records and rows as for dgrp_fasta_extract_batch: record r =
 * bytes [h_off[r], h_off[r] + h_len[r]) of d_raw (16-byte aligned; the ranges ascend and do not overlap), a body with LF or CRLF
 * line ends, sequence position p = the p-th byte that is neither CR nor LF; its rows are d_rows[h_row_off[r] .. h_row_off[r + 1])
 * (device), ascending and disjoint.  The label of a position is the label of the row that covers it, 0 where none does; the kind
 * of a byte is dgrp_encode's class (A,a=0 C,c=1 G,g=2 T,t=3 else 4); a byte is lower case in 'a'..'z'.
 *   d_counts [nrec][C][5][2] int64: positions of record r per (label, kind, lower case);
 *   d_bins   [h_bin_off[nrec]][C] int64 (bin > 0; else unused, may be NULL): row h_bin_off[r] + p / bin is the bin of position p of
 *            record r; column 0 = its ACGT bases (kind < 4), column l >= 1 = its positions under label l.  The host does not know a
 *            record's sequence length (h_len counts the line ends too): h_bin_off[r + 1] - h_bin_off[r] >= ceil(h_len[r] / bin), and
 *            the bins behind the sequence stay 0;
 *   *d_bad   int64: -1, or the smallest index i (into d_rows) of a bad row: a label outside 0..C-1, start < 0, end <= start, end
 *            beyond the record's sequence, or the next row of the record starting below its end.  A bad row is left out of every
 *            count; the call still returns DGRP_OK (a bad row cannot be known without a read-back; the caller reads *d_bad with
 *            the tables).  Where the rows that are left still overlap the counts are unspecified; no access leaves the arrays.
 * The three outputs are zeroed here (*d_bad to -1) on every call.  Everything is enqueued on `stream`: nothing synchronises,
 * copies back or allocates; the host tables are read before the call returns.  Checked first, before any device pointer is
 * touched: the host tables and scalars (DGRP_EINVAL; 2 <= C <= 64, bin >= 0), then the workspace
 * (dgrp_repeat_summary_workspace_bytes of nrec, the sum of h_len and the number of rows; else DGRP_ENOMEM).  nrec == 0: nothing is
 * queued, nothing is written.
 * Stages: sequence bytes per 4096-byte body tile, scanned; one lane per row checks it, the good rows are compacted into the
 * workspace; one lane per tile finds its record, first position, rows and bin; then one workgroup per tile at a time (a
 * workgroup walks consecutive tiles), one aligned 16-byte load per lane: a lane
 * finds the row of its first position by binary search and walks on; counts are summed in an LDS table of C * 10 counters per
 * workgroup (several copies of each, by lane) and flushed with 64-bit integer atomics when the record changes; bin counts go to
 * d_bins with integer atomics (through LDS where a tile lies in one bin).  Integer sums do not depend on their order: the same call
 * gives the same bytes. */
int64_t dgrp_repeat_summary_workspace_bytes(int64_t nrec, int64_t total_bytes, int64_t nrows);
int dgrp_repeat_summary_batch(const uint8_t *d_raw, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                              const dgrp_segment *d_rows, const int64_t *h_row_off, int C, int64_t bin, const int64_t *h_bin_off,
                              int64_t *d_counts, int64_t *d_bins, int64_t *d_bad, void *d_work, int64_t work_bytes, void *stream);

/* ---- A3: deepgrp.prediction.fetch_validation_batch (deepgrp/prediction.py:14-37)
 * Number of windows len(range(0, n - T, s)). */
int64_t dgrp_window_count(int64_t n, int64_t T, int64_t s);
/* Materialise windows w0 .. w0+nw-1 as one-hot [nw, T, 5]; elem = 2 (fp16) or 4 (fp32, what the
 * reference's generator yields).  Not used by the fused path; kept for API parity and as the
 * HBM-roofline probe of the sliding encoder. */
int dgrp_windows_onehot(const uint8_t *d_idx, int64_t n, int64_t T, int64_t s, int64_t w0,
                        int64_t nw, int elem, void *d_out, void *stream);

/* ---- A13: the tensors tf.keras.models.load_model extracts from the HDF5 file
 * (deepgrp/__main__.py:264-270; layer graph deepgrp/model.py:293-336).  Host float32 arrays in
 * Keras layout, gate columns z|r|h:  kernel [5,3u], recurrent [u,3u], bias [2,3u],
 * scale [u] or NULL (no attention), ff_kernel [(attention?2u:u), C], ff_bias [C].
 * Packs them into MFMA fragment order and uploads (synchronous).
 * Sizes: 1 <= u <= 2048, 2 <= C <= 64 (the reference's classes are len(repeats_to_search) + 1 = 5; labels are int8), 1 <= T <= 65535.
 * Up to 256 units and 16 classes the fused kernels run (their logit tile is 16 wide); beyond either, the model is created on the
 * "fp32 path" (dgrp_model_flags bit 2): every forward call goes through the plain-fp32 kernels of ref_kernels.hip, tens of Mbp/s --
 * the reference takes any `units` (deepgrp/model.py:117,219-229), so a large model is slow here, not refused.  Its class probabilities
 * are held to 5e-5 of a float64 evaluation (tests/test_gpu_fp32_path.py: GRU and LSTM, 17-64 classes, up to 2048 units); the largest
 * error measured at 2048 units is 4.1e-7, the same as a CPU fp32 evaluation of those windows. */
int dgrp_model_create(dgrp_model **out, int T, int u, int C, int attention, const float *h_kernel,
                      const float *h_recurrent, const float *h_bias, const float *h_scale,
                      const float *h_ff_kernel, const float *h_ff_bias);
/* rnn = "LSTM" variant (deepgrp/model.py:219-223, no attention): kernel [5,4u], recurrent [u,4u],
 * bias [4u], gate columns i|f|c|o; ff_kernel [u, C], ff_bias [C].  Up to 128 units both kernel sets exist; 129-256 units run the
 * streamed split-operand kernel at either precision level; beyond 256 units the fp32 path, as above. */
int dgrp_model_create_lstm(dgrp_model **out, int T, int u, int C, const float *h_kernel,
                           const float *h_recurrent, const float *h_bias, const float *h_ff_kernel,
                           const float *h_ff_bias);
int dgrp_model_destroy(dgrp_model *m);
int dgrp_model_dims(const dgrp_model *m, int *T, int *u, int *C, int *attention);
/* Which kernel variant the constructor chose (diagnostic; results are the same within tolerance):
 * bit 0 = GRU blend with one reciprocal per (row, unit) -- only when the weights' absolute column sums
 * prove (1 + 2^az)(1 + 2^ag) finite in float32; otherwise (or with DGRP_GRU_SAFE=1 in the environment at
 * construction) the two-reciprocal form; bit 1 = precision level 1 (below); bit 2 = the model runs on the fp32 path (more units
 * than the fused kernels take).  Negative on a NULL model. */
int dgrp_model_flags(const dgrp_model *m);
/* (addition) Precision of the recurrent contraction for every later call on this handle:
 * 1 = split operands, the DEFAULT of every model: weights and hidden state enter the matrix cores as fp16 hi+lo pairs, three MFMA
 * passes, fp32-grade pre-activations -- class probabilities within 1e-5 of a float64 evaluation in the package's tests (GRU up to 64
 * units: gru_wave_kernel; 97-128 units: gru_split2_kernel; other GRU sizes up to 128 units: gru_split_kernel; GRU with 129-256 units
 * and the LSTM cell up to 256 units: rnn_split_stream_kernel).  With attention the recurrent pre-pass runs split and avg[t] crosses to
 * the second kernel as FLOAT32 (fp16 at level 0).
 * 0 = fp16 MFMA operands (`predict --fast`): 2-2.5x faster, class probabilities within 1e-3 of fp32 except on ill-conditioned windows
 * (measure with `python -m deepgrp_amd verify`).  The LSTM cell beyond 128 units and models on the fp32 path (dgrp_model_flags bit
 * 2) have one kernel set and accept either level.  DGRP_EINVAL for any other level.  dgrp_model_flags bit 1 reports the level.
 * The level is a property of the HANDLE, read by every call at launch time: do not change it on a handle other host threads are
 * using -- give each user its own view (dgrp_model_view) instead. */
int dgrp_model_set_precision(dgrp_model *m, int level);
/* (addition) A second handle on the same device-resident model with its own precision level: shares every buffer of `m` (which must
 * outlive it), costs nothing, is released with dgrp_model_destroy.  The package's pipelines hold one view each, so that pipelines of
 * different levels can run records on a pool of host threads without touching each other's setting. */
int dgrp_model_view(const dgrp_model *m, int level, dgrp_model **out);

/* (addition) The recurrent kernel a launch of `mode` (0 merged, 1 window probabilities, 2 attention pre-pass) with step `step`
 * would run on this handle at its current precision level, and its carve (diagnostic; host only, no device work).  *kernel is a
 * DGRP_KERNEL_* value; *lds_bytes the dynamic LDS of the launch (of a workgroup, of a wave for gru_wave_kernel, of one of the two
 * row tiles for gru_split2_kernel); *ospan the rows of the merged-output LDS image (mode 0; 0 = no image, every window merges
 * into HBM); *avg_up the row length of the avg[t] spill (mode 2).  A model on the fp32 path gives DGRP_KERNEL_FP32 and zeros.
 * DGRP_SPLIT_ONE_TILE in the environment is read as by a launch.  DGRP_EINVAL for a NULL argument, a mode outside 0..2,
 * step < 1, or mode 2 on a model without attention. */
#define DGRP_KERNEL_NONE 0       /* the window does not fit the LDS: the launch is refused */
#define DGRP_KERNEL_WAVE 1       /* gru_wave_kernel (GRU up to 64 units, split operands) */
#define DGRP_KERNEL_SPLIT2 2     /* gru_split2_kernel (GRU 97-128 units, split operands) */
#define DGRP_KERNEL_STREAM64 3   /* gru_stream64_kernel (GRU 129-256 units, split operands) */
#define DGRP_KERNEL_STREAM 4     /* rnn_split_stream_kernel (GRU 129-256 units, LSTM) */
#define DGRP_KERNEL_SPLIT 5      /* gru_split_kernel (GRU up to 128 units, split operands) */
#define DGRP_KERNEL_LSTM 6       /* lstm_fused_kernel (LSTM up to 128 units, fp16 operands) */
#define DGRP_KERNEL_FUSED 7      /* gru_fused_kernel (GRU up to 256 units, fp16 operands) */
#define DGRP_KERNEL_FP32 8       /* the plain-fp32 kernels of ref_kernels.hip (dgrp_model_flags bit 2) */
int dgrp_model_plan(const dgrp_model *m, int mode, int64_t step, int *kernel, int64_t *lds_bytes, int *ospan, int *avg_up);

/* ---- A4: model.predict_on_batch (deepgrp/prediction.py:106)
 * Bytes of scratch HBM dgrp_forward_* needs for `nw` windows in one call: the avg[t] spill and the avg half of the logits of an attention
 * model plus 256 bytes, 256 bytes without attention.  One word of it is the launch's queue of tile pairs (gru_split2_kernel, 97-128
 * units: zeroed by the call on its stream), so a workspace belongs to ONE call at a time: calls that run side by side -- other streams,
 * other host threads -- each bring their own.  Without attention the workspace may be NULL / 0 as before: the launch then gives every
 * workgroup a fixed share of the windows instead (same result bit for bit, a few percent slower on records of more than 8 192 windows). */
int64_t dgrp_forward_workspace_bytes(const dgrp_model *m, int64_t nw);
/* Windows per call the library itself uses inside dgrp_predict_record, and the size callers of dgrp_forward_merge should cut a
 * record into (the reference's predict loop, deepgrp/prediction.py:104-110, goes batch by batch; here a "batch" is a launch):
 * 2^23 without attention (a 250 Mbp chromosome at stride 50 in one launch); with attention as many as keep the avg[t] spill of one launch within 1/32 of the card's memory, at most
 * 8 GiB (environment DGRP_SPILL_BYTES overrides), in multiples of 32 768 windows (whole rounds of workgroups for every recurrent
 * kernel) or, below that, of 4096.  0 for a null model. */
int64_t dgrp_forward_window_chunk(const dgrp_model *m);
/* Class probabilities [nw, T, C] float32 of windows w0 .. w0+nw-1 of the index array.  (A workgroup stages its 16
 * windows in LDS: 16 T bytes next to ~25 KiB of state at 128 units, so T up to about 8 000; larger windows are
 * refused with DGRP_EINVAL.) */
int dgrp_forward_windows(const dgrp_model *m, const uint8_t *d_idx, int64_t n, int64_t s,
                         int64_t w0, int64_t nw, float *d_probs, void *d_work, int64_t work_bytes,
                         void *stream);

/* ---- A4+A5+A6 fused: deepgrp.prediction.predict (deepgrp/prediction.py:89-111) with
 * get_max (deepgrp/sequence.pyx:65-76 -> deepgrp/maxcalc.c:10-24) folded into the classifier
 * epilogue.  d_out is float32 [n, C] and MUST be zero-filled by the caller before the first call
 * for a record (np.zeros, prediction.py:103).  Windows w0 .. w0+nw-1 are max-merged at the rows
 * the reference would use for a user batch size `batch` INCLUDING its partial-last-batch
 * offset, computed from the record's total window count. */
int dgrp_forward_merge(const dgrp_model *m, const uint8_t *d_idx, int64_t n, int64_t s,
                       int64_t batch, int64_t w0, int64_t nw, float *d_out, void *d_work,
                       int64_t work_bytes, void *stream);

/* prediction.py:89-111 for a WHOLE record: every window, chunk by chunk (dgrp_forward_window_chunk), max-merged into d_out [n, C],
 * which the caller has zeroed.  Attention models whose chunk is at least 65 536 windows (up to 64 units at the usual window sizes)
 * alternate the chunks between three internal streams ("lanes"), each with a spill of its own: the second kernel of one chunk --
 * HBM-bound -- runs beside the recurrent pre-pass of the next; the caller's stream is forked in front of the first chunk and joined
 * behind the last.  A max-merge: the result does not depend on the order, bit for bit.  dgrp_predict_record runs this. */
int64_t dgrp_forward_merge_record_workspace_bytes(const dgrp_model *m, int64_t n, int64_t s);
int dgrp_forward_merge_record(const dgrp_model *m, const uint8_t *d_idx, int64_t n, int64_t s, int64_t batch, float *d_out,
                              void *d_work, int64_t work_bytes, void *stream);

/* Accuracy yardstick (an addition; no counterpart in the reference, whose TensorFlow graph IS fp32): the same windows
 * through a plain fp32 evaluation of deepgrp/model.py:293-336 on the device -- fp32 weights and state, expf/tanhf, no
 * fp16, no MFMA -- so that the deviation of the fp16-operand fused kernel can be measured on the caller's own weights
 * and sequence (`python -m deepgrp_amd verify`).  Slow (one workgroup per window and strand); meant for hundreds of
 * windows.  Nothing on the prediction path calls it. */
int64_t dgrp_forward_reference_workspace_bytes(const dgrp_model *m, int64_t nw);
int dgrp_forward_windows_reference(const dgrp_model *m, const uint8_t *d_idx, int64_t n, int64_t s, int64_t w0,
                                   int64_t nw, float *d_probs, void *d_work, int64_t work_bytes, void *stream);

/* ---- A6 standalone: float *_get_max(float *output, float *inputs, size_t dim0, size_t dim1,
 * size_t stride, size_t batchsize)  (deepgrp/maxcalc.h:3-4).  Same argument meaning; buffers on
 * the device; out_rows bounds the writes (the reference has no bounds check). */
int dgrp_get_max(float *d_output, int64_t out_rows, const float *d_inputs, int64_t dim0,
                 int64_t dim1, int64_t stride, int64_t batchsize, void *stream);

/* ---- A7: the score transform of deepgrp.prediction.apply_mss (deepgrp/prediction.py:51-57)
 * probs float32 [n, C] -> scores float64 [n] and classes int8 [n] (argmax, first maximum). */
int dgrp_scores(const float *d_probs, int64_t n, int C, double *d_scores, int8_t *d_cls,
                void *stream);
/* ---- A8: deepgrp.prediction.softmax + argmax (deepgrp/prediction.py:62-65,
 * deepgrp/__main__.py:81-83): labels int8 [n]; d_softmax (float32 [n, C]) may be NULL. */
int dgrp_softmax_labels(const float *d_probs, int64_t n, int C, float *d_softmax, int8_t *d_labels,
                        void *d_work, int64_t work_bytes, void *stream);

/* ---- A9+A10: deepgrp.mss.find_mss_labels (deepgrp/_mss/pymss.pyx:16-80) over
 * msseg_t *mss_find_all(int n, const double *S, double min_sc, double xdrop, int *n_seg)
 * (deepgrp/_mss/mss.h:16-17).  scores float64 [n], labels int8 [n] in; labels int8 [n] out (the
 * argmax of the reference's one-hot rows).  n < 2^31 like the reference.  If d_nseg != NULL it
 * receives the number of maximal segments kept (device int64).  Synchronises the stream INSIDE the
 * call (the fixed-point loop over independently scanned stretches reads a flag back); the vote that
 * writes d_labels_out and d_nseg is enqueued behind that: stream-ordered, not complete on return. */
int64_t dgrp_mss_workspace_bytes(int64_t n);
int dgrp_mss_labels(const double *d_scores, const int8_t *d_cls, int64_t n, int nof_labels,
                    int min_mss_len, int xdrop_len, int8_t *d_labels_out, int64_t *d_nseg,
                    void *d_work, int64_t work_bytes, void *stream);
/* The segments themselves (st, en as int32 pairs, in order) for the last dgrp_mss_labels call on
 * this workspace: copies up to cap pairs to the host, returns the count via *n_seg (synchronous:
 * it has no stream argument and waits for all work on the device first, so it may follow a
 * dgrp_mss_labels call on any stream, non-blocking ones included). */
int dgrp_mss_segments_host(const void *d_work, int64_t work_bytes, int32_t *h_st_en, int64_t cap,
                           int64_t *n_seg);

/* The same for MANY records side by side (files of thousands of short records): record r occupies
 * [h_start[r], h_start[r+1]) of d_scores / d_cls / d_labels_out, every start a multiple of 64, h_start[nrec] =
 * total_n < 2^31; positions between a record's last base and the next start must hold score 0.0 and class 0 (they
 * behave like the end of the sequence, deepgrp/_mss/mss.c:96).  One wave per record, one launch per kernel for all
 * of them; synchronises the stream. */
int64_t dgrp_mss_batch_workspace_bytes(int64_t total_n, int64_t nrec);
int dgrp_mss_labels_batch(const double *d_scores, const int8_t *d_cls, int64_t total_n, int64_t nrec,
                          const int64_t *h_start, int nof_labels, int min_mss_len, int xdrop_len,
                          int8_t *d_labels_out, void *d_work, int64_t work_bytes, void *stream);

/* ---- A11: deepgrp.sequence.yield_segments / get_segments (deepgrp/sequence.pyx:38-53,
 * :79-85) filtered by label > 0 (deepgrp/__main__.py:290): run-length extraction with the
 * "last element is its own segment" behaviour.  Writes up to cap records (device) and the total
 * count (device int64; may exceed cap, in which case only cap were written). */
int64_t dgrp_segments_workspace_bytes(int64_t n);
int dgrp_segments(const int8_t *d_labels, int64_t n, int64_t offset, int32_t contig,
                  dgrp_segment *d_records, int64_t cap, int64_t *d_count, void *d_work,
                  int64_t work_bytes, void *stream);

/* ---- A12: the TSV rows of deepgrp/__main__.py:291-292 as text (host code, host buffers): per row
 * "<prefix>start\tend\tlabel\n", prefix i = bytes [prefix_off[i], prefix_off[i+1]) of `prefixes` ("file\theader\t" of record i);
 * a row takes prefix rows[r].contig if by_contig != 0, else prefix 0.  out capacity >= dgrp_format_rows_bound(nrows, longest
 * prefix); *written = bytes produced. */
int64_t dgrp_format_rows_bound(int64_t nrows, int64_t longest_prefix);
int dgrp_format_rows(const char *prefixes, const int64_t *prefix_off, int64_t nprefix, int by_contig,
                     const dgrp_segment *rows, int64_t nrows, char *out, int64_t cap, int64_t *written);

/* ---- probability tracks (an addition, predict --track_dir; the reference writes no probabilities): class `cls` of ONE record's
 * merged probabilities d_probs [n, C] float32 (device) as 4-column bedGraph text "name\tstart\tend\tvalue\n" in d_text (device).
 * Row i of d_probs is record coordinate offset + i (offset = startpos).  Bin k is [k * bin, (k + 1) * bin) of those coordinates,
 * clipped to [offset, offset + n); its value is the maximum of the class column over the bin's rows (starting from 0: a NaN never
 * wins), quantised to q = floor(v * 10^digits + 0.5) in float32 (two roundings) and clamped to [0, 10^digits].  Consecutive bins of
 * equal q are one line; lines of q = 0 are left out.  The value is printed from the integer: q / 10^digits with exactly `digits`
 * decimals ("0.05", "1.00").  name = name_len raw bytes (host), written as they are; up to DGRP_TRACK_NAME_ROOM of them, a longer
 * name is refused (DGRP_EINVAL).  *h_bytes (host) = the text's length, also when it exceeds cap: then nothing is written and the
 * caller retries with a larger buffer.  digits 1..4, bin >= 1, n, offset and bin up to 2^40, and at most 2^39 bins in one call (the
 * grids of the chain; "too many bins in one call" beyond that, and the workspace query gives 0).  This is the batched entry below
 * with one record and one class: the same kernels, the same launch sequence.  Workspace dgrp_track_workspace_bytes(n, bin): the
 * batched layout for one record of at most n / bin + 2 bins, whatever its offset, and a name of DGRP_TRACK_NAME_ROOM bytes -- 4
 * bytes per bin rounded up to tiles of 2048 bins, 8 bytes per tile, and the tables.  Synchronises the stream (at most twice). */
#define DGRP_TRACK_NAME_ROOM 65536     /* bytes: two orders of magnitude above any first word of a FASTA header */
int64_t dgrp_track_workspace_bytes(int64_t n, int64_t bin);
int dgrp_track_text(const float *d_probs, int64_t n, int C, int cls, int digits, int64_t bin, int64_t offset,
                    const char *name, int64_t name_len, char *d_text, int64_t cap, int64_t *h_bytes,
                    void *d_work, int64_t work_bytes, void *stream);

/* The same text for a BATCH of records and several classes in one chain (files of thousands of short records).  Record r is rows
 * [h_row0[r], h_row0[r] + h_n[r]) of d_probs [*, C] (any layout: the rows of dgrp_predict_batch_probs, or one record at row 0), its
 * coordinates start at h_startpos[r], and its first column is names[h_name_off[r] : h_name_off[r + 1]] (raw host bytes).  The
 * output is class-major: d_text[h_class_off[k] : h_class_off[k + 1]] is the text of class h_cls[k] of record 0, then record 1, ...
 * -- exactly the bytes the one-record entry gives record by record, concatenated (a run never crosses a record boundary).
 * h_class_off (host, ncls + 1 entries) is always filled in full, also when h_class_off[ncls] > cap: then nothing is written and the
 * caller retries with a larger buffer.  Format, quantisation, bin alignment and limits as above; ncls in 1..C, classes in 0..C-1,
 * h_n[r] >= 1, ascending h_name_off.  nrec = 0: zero offsets, no device work.  Workspace
 * dgrp_track_batch_workspace_bytes (0 on arguments the entry refuses; names_bytes = h_name_off[nrec]).  Synchronises the stream (at
 * most twice per call, however many records and classes); the host tables may be dropped on return. */
int64_t dgrp_track_batch_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls,
                                         int64_t names_bytes);
int dgrp_track_text_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                          const int64_t *h_startpos, const char *names, const int64_t *h_name_off, const int *h_cls, int ncls,
                          int digits, int64_t bin, char *d_text, int64_t cap, int64_t *h_class_off, void *d_work,
                          int64_t work_bytes, void *stream);

/* The tabix index of that text (predict --track_index), in offsets of the text: for the same arguments as dgrp_track_text_batch, the
 * chunks and the 16 kb linear index of every class's slice, from the same bin, count and scan passes and kernels of its own that
 * follow them; the text itself is not written.  A chunk (the rule of htslib's hts_idx_push) is a maximal run of consecutive lines
 * of ONE record with the same bin reg2bin(start, end) of the standard scheme (min_shift 14, depth 5); it never spans two records,
 * even when they share a name.  beg and end are byte offsets inside the class's slice of the text (slice k is d_text[h_class_off[k]
 * : h_class_off[k + 1]] of the text entry): the first byte of its first line and the byte behind its last line.  Chunks are
 * class-major, in the order of the text: those of class h_cls[k] are d_chunks[h_chunk_off[k] : h_chunk_off[k + 1]].  h_chunk_off
 * (host, ncls + 1 entries) is always filled in full, also when h_chunk_off[ncls] > chunk_cap: then nothing is written, d_linear
 * included, and the caller retries with more room.  d_linear is laid out [class k][record r][window w], w = 0 ..
 * (h_startpos[r] + h_n[r] - 1) >> 14 inclusive, so record r of class k starts at k * W + (windows of the records in front of r), W
 * the windows of all records; linear_cap (in elements) must be at least ncls * W.  A value is the slice offset of the first byte of
 * the record's first line whose end is greater than w << 14, or -1 where the record has no such line.  A record that ends above
 * 2^29 (h_startpos[r] + h_n[r] > 536870912, the largest coordinate of a tabix index) is refused with DGRP_EINVAL before any launch;
 * the other limits and refusals are the text entry's.  Workspace dgrp_track_index_workspace_bytes (0 on arguments the entry
 * refuses): the text entry's, then one int64 per record, 40 bytes per tile of 2048 bins and class, and the chunk boundaries.
 * Synchronises the stream (at most three times). */
typedef struct { int64_t beg, end; int32_t rec; uint32_t bin; } dgrp_track_chunk;
int64_t dgrp_track_index_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls,
                                         int64_t names_bytes);
int dgrp_track_index_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                           const int64_t *h_startpos, const char *names, const int64_t *h_name_off, const int *h_cls, int ncls,
                           int digits, int64_t bin, dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_chunk_off,
                           int64_t *d_linear, int64_t linear_cap, void *d_work, int64_t work_bytes, void *stream);

/* dgrp_track_csi_batch (predict --track_index --index_format csi): dgrp_track_index_batch with the depth of the binning scheme as an
 * argument (deepgrp_amd/tabix.py states the CSI format).  depth is 5 or 6, anything else is DGRP_EINVAL on the host.  A line's bin
 * is csi_reg2bin(start, end, depth): level l of 0..depth starts at bin ((1 << 3l) - 1) / 7 and has shift 14 + 3 (depth - l).  The
 * record-end limit is 2^(14 + 3 depth), 2^32 at depth 6: a record that ends above it is refused with DGRP_EINVAL before any launch
 * ("... the largest coordinate of a CSI index of depth D").  Everything else -- arguments, outputs, chunk rule, the 16 kb windows
 * of d_linear and its rule, synchronisation count, workspace layout -- is dgrp_track_index_batch's, whose outputs these are bit for
 * bit at depth 5; that entry is this code at depth 5.  A record near 2^32 has up to 2^18 windows per class in d_linear. */
int64_t dgrp_track_csi_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls,
                                       int64_t names_bytes, int depth);
int dgrp_track_csi_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                         const int64_t *h_startpos, const char *names, const int64_t *h_name_off, const int *h_cls, int ncls,
                         int digits, int64_t bin, int depth, dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_chunk_off,
                         int64_t *d_linear, int64_t linear_cap, void *d_work, int64_t work_bytes, void *stream);

/* ---- bigWig tracks (predict --track_bigwig; deepgrp_amd/bigwig.py states the file format).  The ITEMS of a class are the lines of
 * the text above without the name: (start, end, q) of every maximal run of bins of equal q != 0 inside one record.  An item's value is
 * (float)((double)q / 10^digits), the float32 a reader gets from the text's decimal.
 *
 * dgrp_track_sections_batch: for the arguments of dgrp_track_text_batch (no names), the items as uncompressed bigWig sections.  A
 * section is up to 1024 consecutive items of ONE record: 24 bytes of header (chromId u32 = chrom0 + the record's index r in this call,
 * chromStart u32 = its first item's start, chromEnd u32 = its last item's end, itemStep u32 = 0, itemSpan u32 = 0, type u8 = 1,
 * reserved u8 = 0, itemCount u16), then itemCount items of (start u32, end u32, value f32), little-endian.  The output is class-major,
 * sections back to back in the order record, start: d_out[h_class_off[k] : h_class_off[k + 1]] holds those of class h_cls[k], and
 * d_table[h_section_off[k] : h_section_off[k + 1]] one row for each of them (off: byte offset in d_out, bytes, rec, start, end).
 * h_class_off and h_section_off (host, ncls + 1 entries each) are always filled in full, also when h_class_off[ncls] > cap or
 * h_section_off[ncls] > table_cap: then nothing is written, to either, and the caller retries with room for all of it.  d_out is
 * 4-byte, d_table 8-byte aligned.  chrom0 >= 0 (the records of the file in front of this call).  Limits and refusals are the text
 * entry's, nrec < 2^31, and a record that ends above 2^32 - 1
 * (h_startpos[r] + h_n[r] > 4294967295, the largest coordinate of a bigWig) is refused with DGRP_EINVAL before any launch.
 * Workspace dgrp_track_sections_workspace_bytes (0 on arguments the entry refuses): the text entry's without names, then 24 bytes
 * per record and class.  Synchronises the stream (at most twice). */
typedef struct { int64_t off, bytes; int32_t rec; uint32_t start, end, pad; } dgrp_track_section;
int64_t dgrp_track_sections_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls);
int dgrp_track_sections_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                              const int64_t *h_startpos, const int *h_cls, int ncls, int digits, int64_t bin, int64_t chrom0, char *d_out,
                              int64_t cap, int64_t *h_class_off, dgrp_track_section *d_table, int64_t table_cap, int64_t *h_section_off,
                              void *d_work, int64_t work_bytes, void *stream);

/* dgrp_track_zoom_batch: for the same arguments, the zoom summaries of DGRP_TRACK_ZOOM_LEVELS levels.  Window w of level l of a record
 * is [w * R, (w + 1) * R) of the record's coordinates, R = 16 * bin * 4^l.  A window with a covered base (a base of a bin with q != 0,
 * edge bins counting only their bases inside [startpos, startpos + n)) gives one 32-byte record: chromId u32 = chrom0 + r, chromStart u32 = its
 * first covered base, chromEnd u32 = one past its last, validCount u32 = its covered bases, then as f32 minVal and maxVal = (float)
 * ((double)q / 10^digits) of the smallest and largest q != 0, sumData = (float)((double)(sum of q * bases) / 10^digits) and sumSquares
 * = (float)((double)(sum of q * q * bases) / 10^(2 * digits)), the sums exact in uint64.  Level 0 is computed from the bins, level
 * l + 1 from level l, four windows at a time.  The records of segment s = k * DGRP_TRACK_ZOOM_LEVELS + l (class h_cls[k], level l) are
 * d_out[32 * h_record_off[s] : 32 * h_record_off[s + 1]], in the order record, window; every 1024 of a segment (the last ones: the
 * rest) are one BLOCK with one row of d_table[h_block_off[s] : h_block_off[s + 1]]: off (bytes in d_out), bytes, cls = k, level = l,
 * the first and last record's chromId, the first one's chromStart and the last one's chromEnd.  h_record_off and h_block_off (host,
 * ncls * DGRP_TRACK_ZOOM_LEVELS + 1 entries each) and h_totals (host, ncls entries: covered bases, smallest and largest q != 0, sum of
 * q * bases, sum of q * q * bases; all 0 with nothing covered) are always filled in full; when the records exceed cap (bytes) or the
 * blocks table_cap nothing is written and the caller retries.  d_out is 16-byte, d_table 8-byte aligned; bin <= 2^32.  Otherwise as
 * dgrp_track_sections_batch.  Workspace dgrp_track_zoom_workspace_bytes: the front's, 80 bytes per record, and 40 bytes per window
 * of all levels and classes (3.4 bytes per bin and class on long records).  Synchronises the stream (at most twice). */
#define DGRP_TRACK_ZOOM_LEVELS 10
typedef struct { int64_t off, bytes; int32_t cls, level, rec0, rec1; uint32_t start, end; } dgrp_track_zoom_block;
typedef struct { uint64_t covered, qmin, qmax, sum, sumsq; } dgrp_track_totals;
int64_t dgrp_track_zoom_workspace_bytes(int64_t nrec, const int64_t *h_n, const int64_t *h_startpos, int64_t bin, int ncls);
int dgrp_track_zoom_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                          const int64_t *h_startpos, const int *h_cls, int ncls, int digits, int64_t bin, int64_t chrom0, char *d_out,
                          int64_t cap, int64_t *h_record_off, dgrp_track_zoom_block *d_table, int64_t table_cap, int64_t *h_block_off,
                          dgrp_track_totals *h_totals, void *d_work, int64_t work_bytes, void *stream);

/* dgrp_zlib_compress_batch: nblk blocks of d_in[0, in_bytes), each as one zlib stream (RFC 1950): 78 01, ONE DEFLATE block from the
 * encoder of the BGZF entries below at `level` (0: literals, 1: matches; a stored block where that is smaller, so a stream is never
 * more than 11 bytes longer than its block), and the Adler-32 of the block, big-endian.  Block m is given by row m of a table on the
 * device: d_rows + m * stride holds int64 offset and int64 length (at most 65280 bytes; the rest of a row is the caller's: the
 * tables of the two entries above fit).  The streams are written back to back to d_out, d_sizes[m] (device) = the size of stream m,
 * *h_out_bytes = their total, also when it exceeds out_cap: then nothing is written and DGRP_ENOMEM is returned.  A row that does
 * not lie in the input or is too long: DGRP_EINVAL, nothing written.  An empty block gives the 11-byte stream of an empty stored
 * block.  dgrp_zlib_bound(nblk, in_bytes) always suffices; workspace dgrp_zlib_workspace_bytes(nblk, level), 16-byte aligned (a
 * 65312-byte slot per block, at level 1 four bytes per input byte of a full block more).  The Adler-32 is computed in parallel on
 * the device.  Synchronises the stream once.  dgrp_zlib_compress_host: the same bytes from host tables, serially. */
int64_t dgrp_zlib_bound(int64_t nblk, int64_t in_bytes);
int64_t dgrp_zlib_workspace_bytes(int64_t nblk, int level);
int dgrp_zlib_compress_batch(const uint8_t *d_in, int64_t in_bytes, const void *d_rows, int64_t stride, int64_t nblk, int level,
                             uint8_t *d_out, int64_t out_cap, int64_t *d_sizes, int64_t *h_out_bytes, void *d_work, int64_t work_bytes,
                             void *stream);
int dgrp_zlib_compress_host(const uint8_t *h_in, int64_t in_bytes, const void *h_rows, int64_t stride, int64_t nblk, int level,
                            uint8_t *h_out, int64_t out_cap, int64_t *h_sizes, int64_t *h_out_bytes);

/* ---- A3-A11 in one call: everything deepgrp/__main__.py:46-83 and :288-292 do for ONE record whose class indices
 * (after N stripping, startpos = offset) are in HBM: windows, forward, max-merge with the reference's placement for
 * `batch`, then scores + MSS labels (use_mss != 0; deepgrp/prediction.py:40-59) or softmax + argmax
 * (deepgrp/__main__.py:81-83), then the label > 0 segments.  Writes up to cap records to d_records, the total to
 * *h_count (host; larger than cap means: call again with more room), synchronises the stream.  All intermediates
 * live in d_work (dgrp_record_workspace_bytes); one host thread per stream may run records concurrently. */
int64_t dgrp_record_workspace_bytes(const dgrp_model *m, int64_t n, int64_t s, int use_mss);
int dgrp_predict_record(const dgrp_model *m, const uint8_t *d_idx, int64_t n, int64_t s, int64_t batch,
                        int min_mss_len, int xdrop_len, int use_mss, int64_t offset, int32_t contig,
                        dgrp_segment *d_records, int64_t cap, int64_t *h_count, void *d_work, int64_t work_bytes,
                        void *stream);

/* The same chain for a BATCH of short records in a handful of launches (a file of thousands of contigs): record r =
 * h_n[r] >= 1 class indices at d_idx + h_idx_off[r] (after N stripping, startpos h_startpos[r]); any model (attention
 * spills avg[t] of every window of the batch into the workspace, so batches are small), MSS labels (the -m path goes
 * record by record: its softmax subtracts the record's global maximum).  One GRU / LSTM launch covers the windows
 * of all records, the post-processing runs on the records laid side by side (64-aligned), one wave per record in
 * the MSS scan.  d_records receives the segments of all records in record order, then position order, `contig` =
 * h_contig[r]; *h_count as in dgrp_predict_record.  Synchronises the stream.  Rows (each record rounded up to 64)
 * must stay below 2^31. */
int64_t dgrp_batch_workspace_bytes(const dgrp_model *m, int64_t nrec, const int64_t *h_n, int64_t s);
int dgrp_predict_batch(const dgrp_model *m, const uint8_t *d_idx, int64_t nrec, const int64_t *h_idx_off,
                       const int64_t *h_n, const int64_t *h_startpos, const int32_t *h_contig, int64_t s, int64_t batch,
                       int min_mss_len, int xdrop_len, dgrp_segment *d_records, int64_t cap, int64_t *h_count,
                       void *d_work, int64_t work_bytes, void *stream);

/* dgrp_batch_rows: the rows of a batch's merged array, the sum of h_n[r] rounded up to 64 each; record r starts at the prefix sum of
 * the same terms.  dgrp_predict_batch_probs: dgrp_predict_batch, with the merged probabilities [dgrp_batch_rows, C] float32 written
 * to the caller's d_probs (device) instead of the workspace; padding rows are zero, the segment rows are the same bit for bit. */
int64_t dgrp_batch_rows(int64_t nrec, const int64_t *h_n);
int dgrp_predict_batch_probs(const dgrp_model *m, const uint8_t *d_idx, int64_t nrec, const int64_t *h_idx_off,
                             const int64_t *h_n, const int64_t *h_startpos, const int32_t *h_contig, int64_t s, int64_t batch,
                             int min_mss_len, int xdrop_len, dgrp_segment *d_records, int64_t cap, int64_t *h_count,
                             void *d_work, int64_t work_bytes, void *stream, float *d_probs);

/* ---- N2: evaluation helpers of deepgrp.prediction on label arrays that are already in HBM.
 * deepgrp.prediction.confusion_matrix (deepgrp/prediction.py:204-222): d_cnf int64 [ncls, ncls] (zeroed here),
 * cnf[true, pred] += 1 per base; labels int8 in [0, ncls), ncls <= 64, arrays 16-byte aligned.  *d_bad (device
 * int) is set to 1 if any label falls outside [0, ncls) -- the reference raises IndexError there. */
int dgrp_confusion_matrix(const int8_t *d_true, const int8_t *d_pred, int64_t n, int ncls, int64_t *d_cnf,
                          int *d_bad, void *stream);
/* deepgrp.prediction.filter_segments (deepgrp/prediction.py:244-260): runs of one positive label shorter than
 * min_len become 0.  d_out may be d_labels (the reference works in place). */
int dgrp_filter_segments(const int8_t *d_labels, int8_t *d_out, int64_t n, int64_t min_len, void *stream);

/* ---- evaluate (an addition; the reference scores label arrays on the host, deepgrp/preprocessing.py:9-48 and
 * deepgrp/prediction.py:225-241).  A flat int8 buffer holds the evaluated bases of nrec records back to back: record r is
 * d_labels[h_off[r] .. h_off[r] + h_len[r]) and its first base has the original coordinate h_origin[r] (its startpos).  Its rows
 * are d_rows[h_row_off[r] .. h_row_off[r+1]) (device), in ORIGINAL record coordinates, in any order, overlapping or not, and are
 * clipped to the record.  Every row must satisfy 0 <= start <= end and 1 <= label <= 127: a bad row gives DGRP_EINVAL before
 * anything is written (the check synchronises the stream once).  Work is balanced by clipped length, not by row.
 * dgrp_paint_rows_batch: every base some row covers is set to the SMALLEST label among the rows that cover it; no other byte is
 * written; deterministic (one pass per label present, highest first, plain stores).
 * dgrp_row_hits_batch: d_hits[i] (int64, for i in [h_row_off[0], h_row_off[nrec])) = bases of row i's clipped span whose label
 * in d_labels equals row i's label (exact integer sums).
 * Both take a workspace of dgrp_eval_workspace_bytes(nrec, rows) bytes. */
int64_t dgrp_eval_workspace_bytes(int64_t nrec, int64_t nrows);
int dgrp_paint_rows_batch(int8_t *d_labels, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                          const dgrp_segment *d_rows, const int64_t *h_row_off, void *d_work, int64_t work_bytes, void *stream);
int dgrp_row_hits_batch(const int8_t *d_labels, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                        const dgrp_segment *d_rows, const int64_t *h_row_off, int64_t *d_hits, void *d_work, int64_t work_bytes,
                        void *stream);

/* ---- scored rows (an addition, predict --bed_dir; the reference reports no confidence per element): for every row, exact integer
 * statistics of its label's column of the merged probabilities over its clipped span.
 * Records as for dgrp_track_text_batch: record r is rows [h_row0[r], h_row0[r] + h_n[r]) of d_probs [*, C] float32 (device; the rows
 * of dgrp_predict_batch_probs, or one record at row 0), its row i has the coordinate h_startpos[r] + i.  Rows as for
 * dgrp_row_hits_batch: record r's rows are d_rows[h_row_off[r] .. h_row_off[r+1]) (device), in ORIGINAL coordinates, in any order,
 * overlapping or not, each clipped to its record.  d_scores[i] is written for i in [h_row_off[0], h_row_off[nrec]), nothing else is.
 * The fixed-point value q(p) of a float32 p: 0 when !(p > 0) (NaN, zero, negatives); else with x = (double)p * 2^24, 2^24 when
 * x >= 2^24, else (uint32_t)floor(x + 0.5) (exact in double).  With L the row's label, over the `bases` rows i of its clipped span:
 * sum = sum of q(P[i, L]), qmin = the smallest q(P[i, L]), agree = the number of i whose first-maximum column is L (best = 0; for c
 * in 1 .. C-1: if P[i, c] > P[i, best] then best = c -- raw floats, a NaN never wins).  bases == 0 gives all zeros; pad is 0.
 * Every statistic is an integer sum, minimum or count: the result does not depend on the grid, on timing or on summation order.
 * Work is shared out by clipped length, not by row: a workgroup takes 8192 positions of the scanned lengths, gathers its rows'
 * partial results in LDS and adds them to d_scores with at most two 64-bit atomic adds (sum, agree) and one 32-bit atomic minimum
 * per (workgroup, row).
 * DGRP_EINVAL before anything is written unless 2 <= C <= 64, h_n[r] >= 1, h_row0[r] >= 0, h_startpos[r] >= 0, h_row_off ascending
 * from a value >= 0, and every row has 0 <= start <= end and 1 <= label < C (that check runs on the device and synchronises the
 * stream once).  DGRP_ENOMEM for a workspace below dgrp_row_scores_workspace_bytes(nrec, rows).  nrec == 0 or no rows: no device
 * work.  After the row check the entry is stream-ordered: the scores are complete behind it on `stream`, not on return. */
typedef struct { uint64_t sum; int64_t bases; int64_t agree; uint32_t qmin; uint32_t pad; } dgrp_row_score;   /* 32 bytes */
int64_t dgrp_row_scores_workspace_bytes(int64_t nrec, int64_t nrows);
int dgrp_row_scores_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                          const int64_t *h_startpos, const dgrp_segment *d_rows, const int64_t *h_row_off,
                          dgrp_row_score *d_scores, void *d_work, int64_t work_bytes, void *stream);

/* ---- probability histograms (an addition, evaluate --curves): per class, the histogram of the merged probability over the
 * evaluated bases, split by whether the base's truth is that class.  Every threshold curve is a function of these integers.
 * Records as for dgrp_row_scores_batch: record r is rows [h_row0[r], h_row0[r] + h_n[r]) of d_probs [*, C] float32 (device); its
 * truth is bytes [h_off[r], h_off[r] + h_n[r]) of d_truth (device int8, as dgrp_paint_rows_batch lays its records).
 * For every base b of every record and every class c, with p = P[b, c] and t the base's truth byte:
 *   k = min(bins - 1, (int)(p * (float)bins))   -- ONE float32 product rounded to nearest, truncated; no reciprocal, no double --
 *   d_hist[c][t == c][k] += 1                    (d_hist: device int64 [C][2][bins], 8-byte aligned; -0.0 counts as 0)
 * A probability that is NaN or outside [0, 1] sets *d_bad (device int) to 1 and that element is not counted; a truth byte outside
 * 0..C-1 sets it too and none of the base's C elements is counted.  The call still returns DGRP_OK (dgrp_confusion_matrix's
 * convention).  d_hist and *d_bad are zeroed here on every call; sums are integers (32-bit counters in LDS, sized so that none can
 * wrap, flushed with 64-bit atomic adds): two calls give the same bytes.  Stream-ordered throughout: nothing synchronises.
 * The kernel reads the flat array once, 4 C + 1 bytes per base, while the classes' counters fit the LDS of one workgroup:
 * C * (8 * bins + 512) + 4096 <= 163840 (C <= 18 at 1000 bins, C <= 4 at 4096); beyond that the classes are cut into the largest
 * groups that fit, and every group reads the array.
 * DGRP_EINVAL before any device work unless 1 <= C <= 64, 2 <= bins <= 4096, nrec >= 0, every h_row0[r], h_n[r], h_off[r] in
 * [0, 2^40), d_hist and d_bad non-NULL, d_hist 8-byte aligned and -- where some record has a base -- d_probs, d_truth and d_work
 * non-NULL and work_bytes >= dgrp_prob_hist_workspace_bytes(nrec, C, bins) (0 for arguments outside the envelope).  nrec == 0 or
 * no base: d_hist and *d_bad are zeroed, nothing else runs. */
int64_t dgrp_prob_hist_workspace_bytes(int64_t nrec, int C, int bins);
int dgrp_prob_hist_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                         const int8_t *d_truth, const int64_t *h_off, int bins, int64_t *d_hist, int *d_bad,
                         void *d_work, int64_t work_bytes, void *stream);

/* ---- strata (an addition, evaluate --strata): which annotated element a base belongs to, and the true class's probability by that.
 * dgrp_paint_strata_batch.  Records and rows as for dgrp_paint_rows_batch, the track being uint32 (4-byte aligned): record r is
 * d_keys[h_off[r] .. h_off[r] + h_len[r]); h_off has nrec + 1 entries here, h_off[nrec] is the size of the track, every record
 * lies inside it, and EVERY element of d_keys[0 .. h_off[nrec]) is written.  d_row_stratum[i] (device uint8) is the stratum of row
 * d_rows[i], i in [h_row_off[0], h_row_off[nrec]).  A base that no row covers gets 0xFFFFFFFF; every other base the SMALLEST
 * label << 8 | stratum among the rows that cover it -- so key >> 8 is the label dgrp_paint_rows_batch paints there, and among the
 * rows of that label the lowest stratum wins.  A fill, then one pass of 32-bit atomic minima over the clipped spans, balanced by
 * length: a minimum does not depend on order, the same call gives the same bytes.  The rows are checked as dgrp_paint_rows_batch
 * checks them (one kernel, one synchronisation of the stream): DGRP_EINVAL before anything is written unless every row has
 * 0 <= start <= end and 1 <= label <= 63.  Workspace: dgrp_eval_workspace_bytes(nrec, rows), DGRP_ENOMEM below it.
 * dgrp_prob_hist_strata_batch.  d_probs, h_row0, h_n as dgrp_prob_hist_batch takes them; record r's keys are d_keys[h_off[r] ..
 * h_off[r] + h_n[r]).  For every base b with a key other than 0xFFFFFFFF, with t = key >> 8, s = key & 255 and p = P[b, t]:
 *   k = min(bins - 1, (int)(p * (float)bins))   -- the bin rule of dgrp_prob_hist_batch --
 *   d_hist[t][s][k] += 1                         (d_hist: device int64 [C][S][bins], 8-byte aligned)
 * t >= C, s >= S, or a p that is NaN or outside [0, 1], sets *d_bad (device int) to 1 and the base is not counted; the call still
 * returns DGRP_OK.  d_hist and *d_bad are zeroed here on every call.  32-bit counters in LDS, sized so that none can wrap, flushed
 * with 64-bit atomic adds: two calls give the same bytes.  Stream-ordered throughout: nothing synchronises.  Where C * S * bins
 * counters exceed 160 KiB of LDS the (class, stratum) cells are cut into groups of 40960 / bins and every group makes a pass: it
 * reads the 4 bytes of key of every base and the float of the bases whose cell it owns; the bytes do not depend on the cut.
 * DGRP_EINVAL before any device work unless 1 <= C <= 64, 1 <= S <= 256, 2 <= bins <= 1000, nrec >= 0, every h_row0[r], h_n[r],
 * h_off[r] in [0, 2^40), d_hist and d_bad non-NULL, d_hist 8-byte aligned and -- where some record has a base -- d_probs, d_keys
 * and d_work non-NULL; DGRP_ENOMEM for work_bytes < dgrp_prob_hist_strata_workspace_bytes(nrec).  nrec == 0 or no base: d_hist
 * and *d_bad are zeroed, nothing else runs. */
int dgrp_paint_strata_batch(uint32_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                            const dgrp_segment *d_rows, const int64_t *h_row_off, const uint8_t *d_row_stratum, void *d_work,
                            int64_t work_bytes, void *stream);
int64_t dgrp_prob_hist_strata_workspace_bytes(int64_t nrec);
int dgrp_prob_hist_strata_batch(const float *d_probs, int C, int64_t nrec, const int64_t *h_row0, const int64_t *h_n,
                                const uint32_t *d_keys, const int64_t *h_off, int S, int bins, int64_t *d_hist, int *d_bad,
                                void *d_work, int64_t work_bytes, void *stream);

/* ---- detection scores (an addition, evaluate --curves --curve_elements): for every annotation row the largest
 * `predict --bed_min_score` m at which the predicted rows that survive m still cover enough of it.  Records are laid out as for
 * dgrp_paint_rows_batch, the track being uint16 (2-byte aligned): record r is d_keys[h_off[r] .. h_off[r] + h_len[r]), its first
 * base has the coordinate h_origin[r]; rows in ORIGINAL coordinates, clipped to their record; labels 1..63.  Both entries take a
 * workspace of dgrp_row_detect_workspace_bytes(nrec, rows) bytes (DGRP_ENOMEM below it) and run one check kernel before anything is
 * written, which synchronises the stream once; behind it they are stream-ordered.  nrec == 0 or no rows: no device work.
 * dgrp_paint_row_keys_batch: every base in the clipped span of predicted row i (d_pred[h_pred_off[r] .. h_pred_off[r+1]) for record
 * r, d_scores[i] its score) is set to key = label << 10 | score, score = R(sum, bases * 2^24, 1000), the integer 0..1000 of BED
 * column 5 (below).  No other element of d_keys is written: the caller zeroes the track.  DGRP_EINVAL, nothing written, for a row
 * with start < 0, end < start or a label outside 1..63; for a row with a base inside its record whose score is outside what
 * dgrp_row_scores_batch writes (0 < bases < 2^40, sum <= bases * 2^24, 0 <= agree <= bases) -- rows without such a base are ignored
 * whatever their score --; and for a row that starts below the end of the row in front of it in its record (predict's rows ascend
 * and do not overlap, so one pass of plain stores paints them).
 * dgrp_row_detect_batch: for annotation row j (d_true[h_true_off[r] .. h_true_off[r+1]); any order, overlapping, nested, sticking
 * out of the record) with label L and clipped span S, hits_m(j) = #{b in S : (L << 10 | m) <= key[b] < ((L + 1) << 10)}.
 * d_detect[j] (int32) = the largest m in 0..1000 with hits_m(j) >= d_need[j] (device int64, the caller's ceil(min_overlap * |S|));
 * -1 when hits_0(j) < d_need[j], when d_need[j] <= 0 or when S is empty.  Written for j in [h_true_off[0], h_true_off[nrec]),
 * nowhere else; d_need is read there only.  hits_m cannot rise with m, so the entry bisects: ten passes over the clipped spans,
 * balanced by length as dgrp_row_hits_batch is, 2 bytes read per base and pass; integer sums, the same bytes on every run. */
int64_t dgrp_row_detect_workspace_bytes(int64_t nrec, int64_t nrows);
int dgrp_paint_row_keys_batch(uint16_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                              const dgrp_segment *d_pred, const int64_t *h_pred_off, const dgrp_row_score *d_scores, void *d_work,
                              int64_t work_bytes, void *stream);
int dgrp_row_detect_batch(const uint16_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                          const dgrp_segment *d_true, const int64_t *h_true_off, const int64_t *d_need, int32_t *d_detect,
                          void *d_work, int64_t work_bytes, void *stream);

/* The scored rows as BED text (host code, host buffers): per row "name\tstart\tend\tclass<label>\tscore\t.\tmean\tmin\tagree\n".
 * name i = bytes [name_off[i], name_off[i+1]) of `names`; a row takes name rows[r].contig if by_contig != 0, else name 0 (the rule
 * of dgrp_format_rows).  With R(num, den, k) = floor((2 k num + den) / (2 den)), integer round-half-up evaluated in 128 bits:
 * score = R(sum, bases * 2^24, 1000), an integer 0..1000 (BED column 5); mean = R(sum, bases * 2^24, 10000), min = R(qmin, 2^24,
 * 10000) and agree = R(agree, bases, 10000), each printed "d.dddd".  Rows with score < min_score are left out.  A row with
 * bases <= 0 gives DGRP_EINVAL.  out capacity >= dgrp_format_bed_bound(nrows, longest name), else DGRP_ENOMEM; *written = bytes
 * produced. */
int64_t dgrp_format_bed_bound(int64_t nrows, int64_t longest_name);
int dgrp_format_bed_rows(const char *names, const int64_t *name_off, int64_t nnames, int by_contig,
                         const dgrp_segment *rows, const dgrp_row_score *scores, int64_t nrows, int min_score,
                         char *out, int64_t cap, int64_t *written);

/* dgrp_bed_text_batch (predict --bed_gzip): the same text written on the device, for rows and scores that are there already
 * (d_rows, d_scores: device; the scores of dgrp_row_scores_batch on the same stream).  names, name_off, nnames and by_contig as
 * above: host tables, staged on the stream, which may be dropped on return.  d_text (device) receives exactly the bytes
 * dgrp_format_bed_rows gives for the same arguments, rows with score < min_score left out.  *h_bytes (host) = the text's length,
 * always; when it exceeds cap nothing is written and the caller retries (dgrp_format_bed_bound(nrows, longest name) never needs
 * that).  One check kernel runs before any byte is written: a row with bases <= 0, or with by_contig a contig outside
 * 0..nnames-1, gives DGRP_EINVAL and leaves d_text untouched.  R is evaluated in 64 bits: with sum = a * bases + r,
 * R(sum, bases * 2^24, k) = (2 k a + 2^24 + floor(2 k r / bases)) >> 25; that holds for what dgrp_row_scores_batch writes, and a
 * row outside it (bases >= 2^40, sum > bases * 2^24, agree outside 0..bases) is refused with DGRP_EINVAL as well.  nrows == 0: no
 * device work, *h_bytes = 0.  nrows < 2^31 - 256.  Workspace dgrp_bed_text_workspace_bytes(nrows, nnames, names_bytes =
 * name_off[nnames]) (0 on arguments the entry refuses): 16 bytes per row, the names and 8 bytes per name; DGRP_ENOMEM when smaller.
 * Synchronises the stream ONCE, for the read-back of the length and the check's flags; the write kernel is enqueued behind it: the
 * text is complete behind the call on `stream`, not on return. */
int64_t dgrp_bed_text_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes);
int dgrp_bed_text_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                        const dgrp_row_score *d_scores, int64_t nrows, int min_score, char *d_text, int64_t cap, int64_t *h_bytes,
                        void *d_work, int64_t work_bytes, void *stream);

/* dgrp_bed_index_batch (predict --bed_index): the tabix pieces of the text dgrp_bed_text_batch writes for the same arguments, in
 * offsets of that text; the text itself is not written.  The record of a row is its contig with by_contig, else 0 (then nrec must
 * be 1); h_rec_end[r] (host, nrec entries) is the end coordinate of record r.
 * Chunks (dgrp_track_chunk, the rule of dgrp_track_index_batch): a maximal run of consecutive EMITTED lines of one record with the
 * same bin reg2bin(start, end), from the first byte of its first line to the byte behind its last line.  A filtered row neither
 * starts nor breaks a run; a chunk never spans two records.  *h_nchunks (host) is always their number; when it exceeds chunk_cap
 * nothing is written, d_linear and d_rec_last included, and the caller retries.
 * d_linear is laid out [record r][window w], w = 0 .. (h_rec_end[r] - 1) >> 14: the text offset of the first emitted line of the
 * record, in file order, whose end is greater than w << 14, or -1 -- the running maximum of the ends decides, so a line that ends
 * below an earlier line of its record claims no window.  linear_cap (elements) must cover the windows of all records.  One thread
 * per window searches the running maximum; a line's windows are never walked.  d_rec_last (device, nrec entries, may be NULL):
 * the end of the record's last emitted line, 0 without one (a tabix index ends a sequence's linear index with its last line).
 * DGRP_EINVAL before anything is written: h_rec_end[r] outside 1..2^29; a row with start < 0, start >= end or end > h_rec_end of
 * its record (or a record outside 0..nrec-1); records that do not ascend with the rows; starts that descend inside a record (every
 * row counts, filtered or not); and the text entry's refusals.  nrows == 0: *h_nchunks = 0, no device work, nothing written.
 * Workspace dgrp_bed_index_workspace_bytes(nrows, nnames, names_bytes, nrec): the text entry's, 76 bytes per row more and 16 per
 * record.  Synchronises the stream ONCE (the read-back of the chunk count and the flags); chunks, linear index and d_rec_last are
 * complete behind the call on `stream`. */
int64_t dgrp_bed_index_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t nrec);
int dgrp_bed_index_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                         const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end,
                         dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear, int64_t linear_cap,
                         int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream);

/* ---- GFF3 (predict --bed_gff3; deepgrp_amd/gff.py states the file format).  The rows and scores of dgrp_bed_text_batch as GFF3
 * feature lines, one per emitted row (score >= min_score), in row order:
 *   seqid \t deepgrp \t repeat_region \t start+1 \t end \t mean \t . \t . \t ID=r<j>;Name=<cname>;label=<L>;score=<score>;min=<min>;agree=<agree> \n
 * score, mean, min and agree are the four figures of the BED line, the same R and the same envelope; seqid is name rows[r].contig
 * (by_contig) or name 0; j = id0 + the 1-based ordinal of the line among the emitted lines of this call (id0: the lines the file
 * holds in front of this text); cname is entry label - 1 of the class-name table (cnames, cname_off, ncnames: laid out like the
 * names), or "class<label>" when ncnames == 0.  Names and class names are copied verbatim: the caller has escaped them.  The
 * "##gff-version 3" line is not written here.  Both tables are host memory, staged on the stream, and may be dropped on return.
 *
 * dgrp_gff_text_batch keeps the contract of dgrp_bed_text_batch: one check kernel before any byte is written; DGRP_EINVAL with
 * d_text untouched for that entry's refusals and for a label outside 1..ncnames when ncnames > 0; refused on the host: id0 outside
 * 0..2^62, descending class-name offsets, a NULL table with ncnames > 0.  *h_bytes (the text's length) and *h_lines (the emitted
 * lines) are always set on success; when the length exceeds cap nothing is written and the caller retries.  nrows == 0: no device
 * work, both 0.  The chain: check -> emitted flag per row -> scan (the ordinals) -> line length per row -> scan (the offsets) ->
 * ONE synchronisation (totals and flags) -> write, one thread per emitted row.  Integers only, no atomics, nothing allocated.
 * Workspace dgrp_gff_text_workspace_bytes (0 on refused arguments): 32 bytes per row, both tables and 8 bytes per entry of each.
 *
 * dgrp_gff_index_batch: the tabix pieces of that text, in offsets of that text: the outputs, intervals ([start, end) of the row),
 * bins, chunk rule, running-maximum linear rule and refusals of dgrp_bed_index_batch, plus the refusals above.  Behind the line
 * lengths it runs the kernels of dgrp_bed_index_batch. */
int64_t dgrp_gff_text_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes);
int dgrp_gff_text_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                        const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                        int64_t nrows, int min_score, int64_t id0, char *d_text, int64_t cap, int64_t *h_bytes, int64_t *h_lines,
                        void *d_work, int64_t work_bytes, void *stream);
int64_t dgrp_gff_index_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes,
                                       int64_t nrec);
int dgrp_gff_index_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                         const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                         int64_t nrows, int min_score, int64_t id0, int64_t nrec, const int64_t *h_rec_end,
                         dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear, int64_t linear_cap,
                         int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream);

/* dgrp_bed_csi_batch, dgrp_gff_csi_batch (predict --bed_index --index_format csi): dgrp_bed_index_batch and dgrp_gff_index_batch
 * with the depth of the binning scheme as an argument behind h_rec_end (deepgrp_amd/tabix.py states the CSI format).  depth is 5 or
 * 6, anything else is DGRP_EINVAL on the host.  A line's bin is csi_reg2bin(start, end, depth); h_rec_end[r] must lie in
 * 1..2^(14 + 3 depth), 2^32 at depth 6, or the call is refused before any launch ("... the largest coordinate of a CSI index of
 * depth D").  Arguments, outputs, chunk rule, running-maximum linear rule over 16 kb windows, refusals, the one synchronisation and
 * the workspace (the _workspace_bytes twins give the .tbi entries' figures; 0 on another depth) are those entries'; at depth 5 the
 * outputs are theirs bit for bit, and those entries are this code at depth 5. */
int64_t dgrp_bed_csi_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t nrec, int depth);
int dgrp_bed_csi_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const dgrp_segment *d_rows,
                       const dgrp_row_score *d_scores, int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end, int depth,
                       dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear, int64_t linear_cap,
                       int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream);
int64_t dgrp_gff_csi_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes,
                                     int64_t nrec, int depth);
int dgrp_gff_csi_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                       const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                       int64_t nrows, int min_score, int64_t id0, int64_t nrec, const int64_t *h_rec_end, int depth,
                       dgrp_track_chunk *d_chunks, int64_t chunk_cap, int64_t *h_nchunks, int64_t *d_linear, int64_t linear_cap,
                       int64_t *d_rec_last, void *d_work, int64_t work_bytes, void *stream);

/* ---- RepeatMasker listing (predict --bed_rmout; deepgrp_amd/rmout.py states the file format).  The rows and scores of
 * dgrp_bed_text_batch as the lines of a RepeatMasker `.out` file, one per emitted row (score >= min_score), in row order:
 *   "%5d %5s %4s %4s  %-16s %9d %9d %11s +  %-12s %-16s %6d %6d %6s %6d\n" %
 *       (score, "0.0", "0.0", "0.0", name, start + 1, end, "(left)", repeat, class/family, 1, end - start, "(0)", ID)
 * every field max(its width, its digits or bytes) wide, numbers right-aligned, names left-justified, "(left)" with its parentheses
 * inside the 11 columns.  score is the BED line's (the same R, the same envelope); name is name rows[r].contig (by_contig) or name
 * 0; left = h_rec_end[record] - end, h_rec_end[r] (host, nrec entries) the end coordinate of record r (a row's contig with
 * by_contig, else 0: then nrec must be 1); repeat and class/family are entries 2 (label - 1) and 2 (label - 1) + 1 of the
 * class-name table (cnames, cname_off: laid out like the names, TWO entries per label, ncnames labels).  ID = id0 + the number of
 * IDs opened up to and including the line: an emitted row opens an ID unless join_gap >= 0 and the emitted row directly in front of
 * it is of the same record and label and start - its end <= join_gap (join_gap -1: every line its own ID); filtered rows neither
 * join nor break.  Names are copied verbatim; the title lines are not written here.  All tables are host memory, staged on the
 * stream, and may be dropped on return.
 *
 * The contract of dgrp_gff_text_batch: one check kernel before any byte is written; DGRP_EINVAL with d_text untouched for the BED
 * entry's refusals (bases <= 0, figures outside what dgrp_row_scores_batch writes, a contig outside the names or outside
 * 0..nrec-1), a label outside 1..ncnames, a row with start < 0, start >= end or end > h_rec_end of its record, records that do not
 * ascend with the rows.  Refused on the host: h_rec_end[r] outside 1..2^62, id0 outside 0..2^62, join_gap < -1, ncnames < 1, a
 * NULL or descending table, nrows >= 2^31 - 256.  *h_bytes (the text's length), *h_lines (the emitted lines) and *h_ids (the IDs
 * they use) are always set on success; when the length exceeds cap nothing is written and the caller retries.  nrows == 0: no
 * device work, all 0.  The chain: check -> emitted flag per row -> scan (the ordinals; the emitted row in front by a binary search
 * over them) -> head-of-ID flag -> scan (the IDs) -> line length per row -> scan (the offsets) -> ONE synchronisation (totals and
 * flags) -> write, one thread per emitted row.  Integers only, no atomics, nothing allocated.  Workspace
 * dgrp_rmout_text_workspace_bytes (0 on refused arguments): 48 bytes per row, the tables and 8 bytes per entry of each. */
int64_t dgrp_rmout_text_workspace_bytes(int64_t nrows, int64_t nnames, int64_t names_bytes, int64_t ncnames, int64_t cnames_bytes,
                                        int64_t nrec);
int dgrp_rmout_text_batch(const char *names, const int64_t *name_off, int64_t nnames, int by_contig, const char *cnames,
                          const int64_t *cname_off, int64_t ncnames, const dgrp_segment *d_rows, const dgrp_row_score *d_scores,
                          int64_t nrows, int min_score, int64_t nrec, const int64_t *h_rec_end, int64_t join_gap, int64_t id0,
                          char *d_text, int64_t cap, int64_t *h_bytes, int64_t *h_lines, int64_t *h_ids, void *d_work,
                          int64_t work_bytes, void *stream);

/* ---- bigBed (predict --bed_bigbed; deepgrp_amd/bigbed.py states the file format).  Both entries take the rows and scores of
 * dgrp_bed_text_batch, no names: the record of a row is its contig with by_contig, else 0 (then nrec must be 1); h_rec_end[r] (host,
 * nrec entries, staged on the stream, may be dropped on return) is the end coordinate of record r; a row is EMITTED when its score
 * is at least min_score.  One check kernel runs before any byte is written; DGRP_EINVAL, with every output untouched, for: the
 * text entry's refusals (bases <= 0, with by_contig a contig outside 0..nrec-1, figures outside what dgrp_row_scores_batch writes);
 * a row with start < 0, start >= end or end > h_rec_end of its record; records that do not ascend with the rows; a row whose start
 * lies below the largest end of the rows in front of it in its record -- overlapping rows and descending starts alike, every row
 * counting, filtered or not; rows that touch are fine.  (predict's rows are the runs of a label array and never overlap; the
 * refusal makes the coverage depth 1 by contract.)  Refused on the host before any device work: h_rec_end[r] outside 1..2^32 - 1,
 * nrec outside 1..2^31 - 1, chrom0 < 0 or chrom0 + nrec > 2^32 - 1, nrows >= 2^31 - 256.  nrows == 0: no device work, all counts 0.
 *
 * dgrp_bed_blocks_batch: the emitted rows as bigBed items, back to back in row order: chromId u32 = chrom0 + record, chromStart
 * u32, chromEnd u32, then columns 4-9 of the BED line exactly as dgrp_format_bed_rows prints them, tab-separated, without the line
 * feed, and one zero byte ("class3\t812\t.\t0.8123\t0.4000\t0.9500\0").  An item is at most 60 bytes (12, "class" and an int32 of
 * at most 11 characters, a score of at most 4, ".", three figures of at most 6, 6 and -- for a qmin up to 2^32 - 1 -- 8, five tabs
 * and the zero), so a BLOCK, up to 512 consecutive emitted rows of ONE record, is at most 30720 bytes, far below the 65280 of a
 * dgrp_zlib_compress_batch row.  d_table gets one row per block, in order: off (bytes in d_out), bytes, rec (the record in this
 * call), start (the first item's), end (the last item's), items; offset and length first, 32 bytes: the row table of
 * dgrp_zlib_compress_batch as it comes.  *h_bytes, *h_nblocks and *h_items (host: bytes, blocks and emitted rows) are always
 * filled; when the bytes exceed cap or the blocks table_cap nothing is written and the caller retries.  d_table is 8-byte aligned.
 * Workspace dgrp_bed_blocks_workspace_bytes (0 on arguments the entry refuses): 28 bytes per row, 24 per record.
 * Synchronises the stream ONCE (the read-back of the counts and the flags); items and table are complete behind the call on
 * `stream`, not on return.
 *
 * dgrp_bed_zoom_batch: the coverage of the emitted rows as zoom summaries, the outputs of dgrp_track_zoom_batch with one class
 * (cls 0): window w of level l of a record is [w * R, (w + 1) * R), R = 1024 * 4^l; a window with a covered base gives one 32-byte
 * record: chromId u32 = chrom0 + r, chromStart u32 = its first covered base, chromEnd u32 = one past its last, validCount u32 = its
 * covered bases, minVal = maxVal = 1.0f, sumData = sumSquares = (float)validCount.  h_record_off and h_block_off (host,
 * DGRP_TRACK_ZOOM_LEVELS + 1 entries each) and *h_totals (covered, 1, 1, covered, covered; all 0 with nothing covered) are always
 * filled; blocks of 1024 records, table rows, capacity protocol and alignment as dgrp_track_zoom_batch.  Level 0 has one thread per
 * window, which finds the rows that touch it by two binary searches; no thread walks a row's windows or a record's rows.  Every
 * figure is an integer count until the one conversion of validCount to float: the result does not depend on the grid, on timing
 * or on any order of summation.  Workspace dgrp_bed_zoom_workspace_bytes (0 on arguments the entry refuses): 48 bytes per row, 88
 * per record, and 12.04 bytes per window of all levels (about 16 per level-0 window of 1024 bases on long records).  Synchronises the
 * stream ONCE; records and table are complete behind the call on `stream`. */
typedef struct { int64_t off, bytes; int32_t rec; uint32_t start, end, items; } dgrp_bed_block;   /* 32 bytes */
int64_t dgrp_bed_blocks_workspace_bytes(int64_t nrows, int64_t nrec, const int64_t *h_rec_end);
int dgrp_bed_blocks_batch(int by_contig, const dgrp_segment *d_rows, const dgrp_row_score *d_scores, int64_t nrows, int min_score,
                          int64_t nrec, const int64_t *h_rec_end, int64_t chrom0, char *d_out, int64_t cap, int64_t *h_bytes,
                          dgrp_bed_block *d_table, int64_t table_cap, int64_t *h_nblocks, int64_t *h_items, void *d_work,
                          int64_t work_bytes, void *stream);
int64_t dgrp_bed_zoom_workspace_bytes(int64_t nrows, int64_t nrec, const int64_t *h_rec_end);
int dgrp_bed_zoom_batch(int by_contig, const dgrp_segment *d_rows, const dgrp_row_score *d_scores, int64_t nrows, int min_score,
                        int64_t nrec, const int64_t *h_rec_end, int64_t chrom0, char *d_out, int64_t cap, int64_t *h_record_off,
                        dgrp_track_zoom_block *d_table, int64_t table_cap, int64_t *h_block_off, dgrp_track_totals *h_totals,
                        void *d_work, int64_t work_bytes, void *stream);

/* ---- compressed input (an addition; the reference reads plain text only): DEFLATE (RFC 1951) streams inflated by the
 * same decode core on the device and on the host (deepgrp_amd/csrc/inflate.h).  A stream that cannot be decoded gives
 * DGRP_EDATA and one of these reasons; no read or write leaves the stream's input and output slices. */
#define DGRP_EDATA (-5)                /* corrupt compressed data (reason below)                  */
#define DGRP_INFLATE_OK 0
#define DGRP_INFLATE_EINPUT 1          /* the input ends inside the stream                         */
#define DGRP_INFLATE_EBLOCK 2          /* block type 3                                              */
#define DGRP_INFLATE_ESTORED 3         /* stored block whose LEN and NLEN do not match              */
#define DGRP_INFLATE_ECODES 4          /* over-subscribed, incomplete or malformed code length set  */
#define DGRP_INFLATE_ESYMBOL 5         /* a symbol that no valid stream contains                    */
#define DGRP_INFLATE_EDIST 6           /* a distance before the start of the output                 */
#define DGRP_INFLATE_EOUTPUT 7         /* more output than the slice (ISIZE) allows                 */
#define DGRP_INFLATE_ECRC 8            /* gzip member: CRC-32 differs from its trailer              */
#define DGRP_INFLATE_EISIZE 9          /* gzip member: fewer bytes than its trailer's ISIZE         */
#define DGRP_INFLATE_ETRAIL 10         /* gzip member: the stream ends before the member's trailer  */

/* One raw DEFLATE stream h_in[0, in_len) inflated on the HOST (no device needed): the output goes to h_out[0, out_cap);
 * *h_out_len = bytes produced and *h_in_used = input bytes up to the end of the final block (also on failure: how far it got);
 * *h_reason = DGRP_INFLATE_* (0 on success).  Returns 0, DGRP_EDATA for a bad stream, DGRP_EINVAL for bad arguments
 * (sizes above 2^31 - 1 included).  Synchronous. */
int dgrp_inflate_raw_host(const uint8_t *h_in, int64_t in_len, uint8_t *h_out, int64_t out_cap, int64_t *h_out_len,
                          int64_t *h_in_used, int *h_reason);

/* nmem gzip members of ONE device buffer inflated in one launch (BGZF: up to 64 KiB each).  Member m's DEFLATE data is
 * d_in[h_in_off[m], h_in_off[m] + h_in_len[m]) and its 8-byte trailer (CRC-32, ISIZE, little endian) follows directly; all of it
 * lies inside d_in[0, in_bytes).  Its output is d_out[h_out_off[m], h_out_off[m+1]) (h_out_off: nmem + 1 ascending values, the
 * prefix sum of the ISIZEs, h_out_off[nmem] <= out_bytes, each slice < 2^31).  Every member must end its final block exactly at
 * its trailer and match the trailer's CRC-32 and ISIZE (checked on the device).  On DGRP_EDATA *h_bad = the lowest failing member
 * and *h_reason its DGRP_INFLATE_* reason (bytes of failing members are undefined); on success *h_bad = -1, *h_reason = 0.
 * A member's reason is the first that applies of: the stream's own (1 .. 7), DGRP_INFLATE_ETRAIL, DGRP_INFLATE_EISIZE or
 * DGRP_INFLATE_EOUTPUT (fewer or more bytes than ISIZE), DGRP_INFLATE_ECRC; the members beside a failing one are complete.
 * Workspace dgrp_inflate_workspace_bytes(nmem).  Synchronous (one read-back of the per-member status). */
int64_t dgrp_inflate_workspace_bytes(int64_t nmem);
int dgrp_inflate_batch(const uint8_t *d_in, int64_t in_bytes, int64_t nmem, const int64_t *h_in_off, const int64_t *h_in_len,
                       const int64_t *h_out_off, uint8_t *d_out, int64_t out_bytes, int64_t *h_bad, int *h_reason, void *d_work,
                       int64_t work_bytes, void *stream);

/* ---- plain gzip input: ONE DEFLATE stream inflated as many spans (deepgrp_amd/csrc/inflate_stream.h).  The stream is cut into
 * chunks of chunk_bytes (64 .. 2^28) compressed bytes; in every chunk but the first the first bit offset that looks like the start
 * of a non-final dynamic block is a span start; spans are decoded side by side without the 32 KiB of text in front of them (first
 * counted, then into 16-bit symbols with markers for bytes of that window), a chain from bit 0 confirms the starts and replaces
 * the wrong and the missing ones, and the markers are resolved once the windows are known.  A stream without any such start is one
 * span.  The chain refuses (DGRP_EDATA) a span of more than max_span_bytes (1 .. 2^31 - 64) compressed bytes and a chain that is
 * not closed after max_rounds (>= 1) counting rounds, with these reasons beside the stream errors above: */
#define DGRP_INFLATE_ESPAN 11          /* a span is longer than max_span_bytes                      */
#define DGRP_INFLATE_EROUNDS 12        /* the chain is not closed after max_rounds rounds           */
typedef struct dgrp_inflate_stream_stats {
    int64_t spans;        /* spans of the closed chain                                                                  */
    int64_t candidates;   /* chunks in which the finder found a start                                                   */
    int64_t repaired;     /* starts the chain replaced by the landing of the span in front                              */
    int64_t rounds;       /* counting rounds                                                                            */
    int64_t longest_span; /* compressed bytes of the longest span                                                       */
    int64_t false_starts; /* of `repaired`: a start of the finder in front of the landing, that is, not a block start   */
    int64_t chunks;
    int64_t reserved;
} dgrp_inflate_stream_stats;

/* The whole algorithm on the HOST through the same code (finder, counting pass, chain, symbols, window walk, resolve): the raw
 * DEFLATE stream h_in[0, in_len) into h_out[0, out_cap).  *h_out_len = bytes produced, *h_in_used = input bytes up to the end of the
 * final block (both 0 on failure), *h_reason = DGRP_INFLATE_* (DGRP_INFLATE_EOUTPUT when the text exceeds out_cap; nothing is
 * written then).  Returns 0, DGRP_EDATA, or DGRP_EINVAL for bad arguments.  Needs no device. */
int dgrp_inflate_stream_host(const uint8_t *h_in, int64_t in_len, int64_t chunk_bytes, int64_t max_span_bytes, int max_rounds,
                             uint8_t *h_out, int64_t out_cap, int64_t *h_out_len, int64_t *h_in_used,
                             dgrp_inflate_stream_stats *h_stats, int *h_reason);

/* The same on the DEVICE in two calls, because the output is allocated between them.  The stream is d_in[data_off, in_bytes)
 * (for a gzip member: behind its header; whatever follows the final block, such as the trailer, is not read as stream).
 * scan: finder, counting rounds and chain; *h_total = bytes of text, *h_stats as the host entry gives them (the chain is the same
 * code), and the chain stays in the workspace.  write: the symbols into d_sym[0, out_bytes) (uint16), the text into
 * d_out[0, out_bytes) with out_bytes = *h_total, *h_crc = CRC-32 of the text, *h_in_used = bytes of d_in up to the end of the final
 * block (data_off included), from the chain scan left in the same workspace for the same d_in, in_bytes, data_off and chunk_bytes
 * (anything else in the workspace is DGRP_EINVAL and launches nothing).  Workspace: dgrp_inflate_stream_workspace_bytes(in_bytes,
 * chunk_bytes) (0 for sizes the entries refuse), 256-byte aligned.  Both are synchronous; bad arguments launch nothing. */
int64_t dgrp_inflate_stream_workspace_bytes(int64_t in_bytes, int64_t chunk_bytes);
int dgrp_inflate_stream_scan(const uint8_t *d_in, int64_t in_bytes, int64_t data_off, int64_t chunk_bytes, int64_t max_span_bytes,
                             int max_rounds, int64_t *h_total, dgrp_inflate_stream_stats *h_stats, int *h_reason, void *d_work,
                             int64_t work_bytes, void *stream);
int dgrp_inflate_stream_write(const uint8_t *d_in, int64_t in_bytes, int64_t data_off, int64_t chunk_bytes, uint16_t *d_sym,
                              uint8_t *d_out, int64_t out_bytes, uint32_t *h_crc, int64_t *h_in_used, int *h_reason, void *d_work,
                              int64_t work_bytes, void *stream);

/* ---- compressed output (an addition): n bytes as a BGZF file, the way bgzip lays it out -- members of 0xff00 input bytes (the last
 * one shorter; n = 0: none), each an 18-byte header with BC / BSIZE, ONE DEFLATE block, CRC-32 and ISIZE; with `eof` the empty
 * EOF member (28 bytes) behind them.  The block holds literals under a per-member dynamic Huffman code (no matches), or is a
 * stored block when that is not larger, so a member never exceeds its input by more than 31 bytes.  The encode core
 * (deepgrp_amd/csrc/deflate.h) is the same on the device and on the host: both entries give the same bytes.
 * dgrp_bgzf_bound(n, eof): an output capacity that always suffices.  *h_out_bytes = bytes of the file (on DGRP_ENOMEM: the
 * capacity it needs).  DGRP_EINVAL for negative sizes and NULL pointers with something to read or write; DGRP_ENOMEM when the
 * workspace (dgrp_bgzf_workspace_bytes(n), 16-byte aligned) or the output is too small: the device entry then writes nothing to
 * d_out, the host entry nothing from the first member that does not fit.  d_in may have any alignment.
 * dgrp_bgzf_compress is synchronous (one read-back of the total). */
int64_t dgrp_bgzf_bound(int64_t n, int eof);
int64_t dgrp_bgzf_workspace_bytes(int64_t n);
int dgrp_bgzf_compress(const uint8_t *d_in, int64_t n, uint8_t *d_out, int64_t out_cap, int64_t *h_out_bytes, int eof, void *d_work,
                       int64_t work_bytes, void *stream);
int dgrp_bgzf_compress_host(const uint8_t *h_in, int64_t n, uint8_t *h_out, int64_t out_cap, int64_t *h_out_bytes, int eof);

/* The same file at a chosen level; everything above holds (arguments, capacities, DGRP_ENOMEM, dgrp_bgzf_bound), with the workspace
 * dgrp_bgzf_workspace_bytes_level(n, level).
 *   level 0: the encoder above, byte for byte what dgrp_bgzf_compress / dgrp_bgzf_compress_host write.
 *   level 1: matches.  Per position of a member the candidate is the nearest earlier position IN THE SAME MEMBER whose 4 bytes hash
 *            to the same 15-bit bucket; it is a match when at least 4 bytes agree (up to 258, distance up to 32768, overlap allowed);
 *            the parse is greedy from the member's first byte.  One block under a dynamic literal/length code and a dynamic distance
 *            code.  Per member the smaller of this block and level 0's is written, so no member is larger than at level 0.
 * Both levels are stated once for host and device (deflate.h): the two entries give the same bytes.  Any other level: DGRP_EINVAL
 * (dgrp_bgzf_workspace_bytes_level: 0). */
int64_t dgrp_bgzf_workspace_bytes_level(int64_t n, int level);
int dgrp_bgzf_compress_level(const uint8_t *d_in, int64_t n, uint8_t *d_out, int64_t out_cap, int64_t *h_out_bytes, int eof, int level,
                             void *d_work, int64_t work_bytes, void *stream);
int dgrp_bgzf_compress_host_level(const uint8_t *h_in, int64_t n, uint8_t *h_out, int64_t out_cap, int64_t *h_out_bytes, int eof,
                                  int level);

/* ---- training (deepgrp/training.py and model.compile / model.fit of deepgrp/model.py:293-336; TensorFlow's job in the reference).
 * GRU models only, 1 <= u <= 256, 2 <= C <= 16, 1 <= T <= 4096, 1 <= B <= 2^18.  The parameters are ONE flat float32 device buffer
 * in Keras layout, tensors back to back: kernel [5, 3u], recurrent_kernel [u, 3u], bias [2, 3u], scale [u] (attention only),
 * FF/kernel [(attention ? 2u : u), C], FF/bias [C]; the count is what the param_count entry returns (0 on sizes the step refuses).
 * The gradients have the same layout.
 *
 * dgrp_train_step: window i of the batch is d_idx[d_starts[i] .. + T) (class indices as dgrp_encode writes them, any value above 4
 * read as 4 = N); its truth is d_truth[c * n + d_starts[i] + t], the int8 [C, n] multi-hot array of preprocess_y.  d_starts is a
 * DEVICE array; a start outside [0, n - T] is clamped into it (no access leaves the arrays), starts may repeat.  d_masks [B, 2, 5]
 * float32 are the GRU cell's input dropout masks per (window, direction: 0 the window, 1 its reverse complement, input channel),
 * constant over the steps, 0 or 1 / (1 - rate); NULL = no dropout.  *d_loss (device float) = Keras' CategoricalCrossentropy: the
 * probabilities divided by their sum, clipped to [1e-7, 1 - 1e-7], -sum_c y_c log p_c averaged over the B T positions.  d_grads
 * receives d loss / d parameters (every element written, nothing accumulated); with d_grads NULL only the loss is computed, by the
 * same kernels: the same bits.  A clipped probability has no gradient, as in Keras.  Every sum across threads runs in a fixed
 * order: the same call gives the same bytes.  Stream-ordered: nothing synchronises or reads back.  Workspace
 * dgrp_train_workspace_bytes (0 on sizes the step refuses), 16-byte aligned, DGRP_ENOMEM when smaller.
 * Batch size in practice: the last kernel adds the partial gradients in index order, one thread per parameter over
 * 2 ceil(B / 16) ceil(T / 32) partials (and B for the head's tensors and the loss), so its time grows with B: microseconds at
 * the reference's batch of 256, a serial tail of milliseconds beyond some 10^4 windows.  Sizes up to 2^18 are correct, not fast. */
int64_t dgrp_train_param_count(int u, int C, int attention);
int64_t dgrp_train_workspace_bytes(int T, int u, int C, int attention, int64_t B);
int dgrp_train_step(int T, int u, int C, int attention, const float *d_params, const uint8_t *d_idx, const int8_t *d_truth,
                    int64_t n, const int64_t *d_starts, int64_t B, const float *d_masks, float *d_loss, float *d_grads,
                    void *d_work, int64_t work_bytes, void *stream);

/* dgrp_train_step_multi: up to DGRP_TRAIN_MAX_JOBS independent training steps in ONE chain of launches (a hyper-parameter search
 * trains many small models; one step of one model fills an eighth of the device at the reference's batch of 256).  A job is
 * exactly the argument list of dgrp_train_step, and job k receives the bytes that dgrp_train_step gives for the same arguments
 * whatever else is in the list: *d_loss, d_grads, or the loss alone where its d_grads is NULL.  Jobs may differ in every field,
 * mix loss-only and gradient jobs, and share d_idx / d_truth / d_starts / d_masks; their d_loss, d_grads and workspaces must not
 * overlap (checked for the workspace ranges that the jobs use).  Each job brings its own workspace of dgrp_train_workspace_bytes.
 * Every job is checked as dgrp_train_step checks its arguments BEFORE anything is launched; a refusal names the job
 * ("job 2: training: 257 units outside 1..256") and launches nothing.  h_jobs is a HOST array, read during the call only: the
 * jobs travel in the kernel arguments.  Stream-ordered: nothing synchronises, copies or allocates.  dgrp_train_step is the
 * call with one job. */
#define DGRP_TRAIN_MAX_JOBS 8
typedef struct dgrp_train_job {
    int T, u, C, attention;
    const float *d_params;
    const uint8_t *d_idx;
    const int8_t *d_truth;
    int64_t n;
    const int64_t *d_starts;
    int64_t B;
    const float *d_masks;
    float *d_loss, *d_grads;
    void *d_work;
    int64_t work_bytes;
} dgrp_train_job;
int dgrp_train_step_multi(const dgrp_train_job *h_jobs, int K, void *stream);

/* One optimizer step on `count` float32 parameters, in place, in float32, one rounding per operation as written:
 * DGRP_OPT_RMSPROP  s1 = rho s1 + ((1 - rho) g) g;  s2 = momentum s2 + (lr g) / sqrt(s1 + epsilon);  w = w - s2
 * DGRP_OPT_ADAM     s1 = b1 s1 + (1 - b1) g;  s2 = b2 s2 + ((1 - b2) g) g;  w = w - (lr_t s1) / (sqrt(s2) + epsilon), with b1 = momentum,
 *                   b2 = rho (the mapping of deepgrp/model.py's _get_optimizer) and lr_t = lr sqrt(1 - b2^step) / (1 - b1^step) computed in
 *                   double on the host; step counts from 1.
 * The scalars are rounded to float32 once ((1 - rho) from the double difference).  d_state1 / d_state2: zero before the first step.
 * Stream-ordered. */
#define DGRP_OPT_RMSPROP 0
#define DGRP_OPT_ADAM 1
int dgrp_optimizer_step(int kind, float *d_params, const float *d_grads, float *d_state1, float *d_state2, int64_t count,
                        double learning_rate, double rho, double momentum, double epsilon, int64_t step, void *stream);

/* ---- training data from a sequence file (an addition; the reference prepares these on the host from a one-hot .npz:
 * deepgrp/preprocessing.py:9-70 and deepgrp/training.py:76-132).  A SIDE is the kept records of a file back to back in one buffer of
 * n_total bases: record r is [h_off[r], h_off[r] + h_len[r]), h_len[r] = its bases from the first to the last non-N WITHOUT the last
 * one (drop_start_end_n), and its first base has the original coordinate h_origin[r].  All three entries work on the caller's stream
 * and allocate nothing.
 *
 * The truth entry writes EVERY byte of d_truth, int8 [C, n_total] (16-byte aligned), the multi-hot truth of preprocess_y: record r's
 * rows are d_rows[h_row_off[r] .. h_row_off[r+1]) (device; ORIGINAL coordinates, any order, overlapping or not, clipped to the
 * record); d_truth[label, b .. e) = 1 for every row, so two classes on one base give two ones, and d_truth[0, j] = 1 where no row
 * covers j (also outside every record).  Every row must satisfy 0 <= start <= end and 1 <= label <= C - 1: a bad row gives
 * DGRP_EINVAL naming it BEFORE any byte of d_truth is written (the check runs on the device and synchronises the stream once; without
 * rows nothing synchronises).  Then: rows 1 .. C-1 cleared, one length-balanced paint pass over all rows (the painter of the evaluate
 * entries: 8192 positions per workgroup, every store a 1 on the row's own class row), one pass that writes row 0 from the others.
 * Plain stores, no atomics on d_truth: the same call gives the same bytes.  2 <= C <= 64.  Workspace (256-byte aligned) of the
 * bytes the companion below returns, DGRP_ENOMEM when smaller. */
int64_t dgrp_truth_workspace_bytes(int64_t nrec, int64_t nrows);
int dgrp_truth_multihot_batch(int8_t *d_truth, int C, int64_t n_total, int64_t nrec, const int64_t *h_off, const int64_t *h_len,
                              const int64_t *h_origin, const dgrp_segment *d_rows, const int64_t *h_row_off, void *d_work,
                              int64_t work_bytes, void *stream);

/* The class-set entry: the window starts of ONE class row d_row [n_total] (a row of d_truth) for windows of T bases, 1 <= T <= 4096.
 * Start s of record r is a member when 1 <= s <= h_len[r] - 1 - T and d_row holds a non-zero byte in [s + 1, s + T] of the record
 * -- exactly _calc_indices(row of the record, T); the bytes tested are the record's own.  The members are written ascending as int64
 * BUFFER positions h_off[r] + s, records in order, to d_starts[0 .. *h_count).  The entry SYNCHRONISES the stream once, to return
 * the count in *h_count.  d_starts NULL: count only.  A count above `cap`: DGRP_ENOMEM, *h_count = the capacity needed, d_starts
 * untouched.  A workgroup takes 8192 starts: it stages their 8191 + T bytes in LDS, counts them into a prefix, and a start is a
 * member when the prefix moves over its window; one pass counts per workgroup, the counts are scanned, a second pass writes.
 * Workspace (256-byte aligned) of the bytes the companion below returns. */
int64_t dgrp_class_starts_workspace_bytes(int64_t nrec, int64_t n_total);
int dgrp_class_window_starts(const int8_t *d_row, int64_t n_total, int64_t nrec, const int64_t *h_off, const int64_t *h_len, int T,
                             int64_t *d_starts, int64_t cap, int64_t *h_count, void *d_work, int64_t work_bytes, void *stream);

/* The resolve entry: d_starts[i] (int64, device) for the B picks d_picks [B, 2] int64 (device): (set, rank).  Set k in [0, nsets)
 * is the ascending array d_set_ptr[k] of d_set_size[k] starts (device tables of device pointers and sizes; what the class-set entry
 * wrote); the start is its element `rank`.  Any other set, or an empty one, is the uniform part: with W_r = max(h_len[r] - T, 0),
 * d_wprefix [nrec + 1] the exclusive prefix sums of W_r and d_base[r] = h_off[r], rank k of [0, W) is d_base[r] + k - d_wprefix[r]
 * for the record with d_wprefix[r] <= k < d_wprefix[r + 1] (binary search).  A rank outside its range is clamped into it; with
 * W = 0 the start is 0: no access leaves the arrays.  Stream-ordered: nothing synchronises, copies or allocates.  1 <= B <= 2^18,
 * 0 <= nsets <= 64, nrec >= 1. */
int dgrp_train_resolve_starts(const int64_t *d_picks, int64_t B, const int64_t *const *d_set_ptr, const int64_t *d_set_size,
                              int nsets, const int64_t *d_base, const int64_t *d_wprefix, int64_t nrec, int64_t *d_starts,
                              void *stream);

/* ---- RepeatMasker listings read on the device (an addition; the reference reads them on the host: deepgrp/_scripts/parse_rm.py).
 * d_text [n]: the text of a `.out` listing or a UCSC `rmsk` table in device memory, any alignment.  The entry finds the lines, takes
 * each through the token statement of parse_rm's two patterns (`.out` first, then `rmsk`), numbers it and keeps it when the
 * number is above 0:
 *   number = position (from 1) of the family -- `rmsk`: class, or class/family where they differ -- among the nnames names
 *   d_names[d_name_off[i] .. d_name_off[i + 1]) (device), else of the repeat name, else unit_number for a family `Simple_repeat` or
 *   `Satellite` whose repeat name opens with `(` [ACGT]+ `)n`, the unit a multiple of five long, every 5-mer c of it with
 *   d_pentamers[c] != 0 and one with d_pentamers[c] == 1 (device uint8 [1024], c = the five bases A C G T = 0 1 2 3 as base-4 digits,
 *   first base highest).
 * Kept rows, in file order, i = 0 .. kept - 1: d_begin[i] (`.out`: begin - 1), d_end[i], d_number[i], d_name_pos[i] / d_name_len[i]
 * (the contig token as a span of d_text), d_line[i] (from 1).  d_run_first[r], r = 0 .. runs - 1: the first row of run r, a maximal
 * stretch of rows whose contig tokens are byte-equal.  h_counts[4] (host): lines, kept rows, runs, not-plain flag.
 * NOT PLAIN: a byte outside 0x20..0x7e other than tab and line feed, a carriage return not directly before a line feed, or a
 * coordinate of more than 18 digits.  Then h_counts[3] = 1, no row is written and DGRP_OK is returned: the caller parses such a
 * file on the host.  More kept rows than `cap`: DGRP_ENOMEM, h_counts[1] = the capacity needed, no row written; n / 22 + 1 rows always
 * suffice (the shortest line that matches).  n = 0: zero counts.  Refused before any launch with DGRP_EINVAL: NULL text with n > 0,
 * n < 0, a NULL table, a NULL output with cap > 0; with DGRP_ENOMEM: a workspace (256-byte aligned) below the companion's bytes.
 * A workgroup takes DGRP_RM_TILE_BYTES of text, a lane 128 of them and the lines that start there; a count pass, two scans, a write
 * pass, then the run flags, their scan and the run starts.  Integers only; the only atomic is the OR of the flag: the same call
 * gives the same bytes.  On the caller's stream; it SYNCHRONISES that stream twice (counts, then runs) and allocates nothing. */
#define DGRP_RM_TILE_BYTES 32768
int64_t dgrp_rm_parse_workspace_bytes(int64_t n);
int dgrp_rm_parse(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off, int nnames,
                  const uint8_t *d_pentamers, int unit_number, int64_t *d_begin, int64_t *d_end, int32_t *d_number, int64_t *d_name_pos,
                  int32_t *d_name_len, int64_t *d_line, int64_t *d_run_first, int64_t cap, int64_t *h_counts, void *d_work,
                  int64_t work_bytes, void *stream);
/* dgrp_rm_parse_fields: the same call -- the same counts, the same arrays, the same refusals -- plus d_millidiv[i] (device int32,
 * `cap` elements, non-NULL where cap > 0): the divergence of kept row i from its consensus in tenths of a percent, -1 where the
 * line does not state one.  The line is tokenised once: the pass that finds the row notes the span of the token, the write pass
 * converts it.  `.out` (token 1, percent): the WHOLE token is D, `D.` or `D.d...` with D 1..6 decimal digits and digits only behind
 * the point -> 10 * D + the first digit behind the point (0 if none); further digits are dropped, not rounded.  `rmsk` (field 2,
 * `milliDiv`, digits already): that integer when it has at most 7 digits.  Anything else -- an empty integer part, a sign, an
 * exponent, other characters, more digits -- is -1; parse_rm's pattern accepts any token there, so such a line stays a kept row. */
int dgrp_rm_parse_fields(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off, int nnames,
                         const uint8_t *d_pentamers, int unit_number, int64_t *d_begin, int64_t *d_end, int32_t *d_number,
                         int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line, int64_t *d_run_first, int32_t *d_millidiv,
                         int64_t cap, int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream);

/* dgrp_rm_parse_all: the same two passes with EVERY line that matches one of the two patterns kept as a row, whatever its number:
 * d_number[i] is 0 where the numbering rule above finds none.  The arrays of dgrp_rm_parse_fields, and the family token of row i as
 * spans of d_text: d_fam_pos[i] / d_fam_len[i] (`.out`: token 10; `rmsk`: field 11) and d_fam2_pos[i] / d_fam2_len[i], the second
 * piece of the logical string `field 11` '/' `field 12` where the two fields differ -- length 0 for `.out` and where they are
 * byte-equal (the position is then that of the first span).  The strings are compared in place and never joined.  Its rows with
 * d_number > 0 are the rows of dgrp_rm_parse_fields in the same order with the same values.  Counts, the not-plain flag (a family
 * token the int32 length cannot state raises it too), DGRP_ENOMEM with the need in h_counts[1], the runs, the refusals and the two
 * synchronisations are those of dgrp_rm_parse; n / 22 + 1 rows still suffice.  Workspace: dgrp_rm_parse_all_workspace_bytes(n). */
int64_t dgrp_rm_parse_all_workspace_bytes(int64_t n);
int dgrp_rm_parse_all(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off, int nnames,
                      const uint8_t *d_pentamers, int unit_number, int64_t *d_begin, int64_t *d_end, int32_t *d_number,
                      int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line, int64_t *d_run_first, int32_t *d_millidiv,
                      int64_t *d_fam_pos, int32_t *d_fam_len, int64_t *d_fam2_pos, int32_t *d_fam2_len, int64_t cap, int64_t *h_counts,
                      void *d_work, int64_t work_bytes, void *stream);

/* ---- rows as text read on the device (an addition, `compare`): the table evaluation.read_annotation reads and the TSV
 * `predict` writes.  d_text [n]: the text in device memory, any alignment.  format 0, TABLE: a line is its tokens between runs of
 * blanks (space, tab); a line without a token, or whose first token opens with '#', is skipped; fewer than four tokens make it
 * MALFORMED (reason 1); else it is a row: token 0 the name, tokens 1..3 begin, end, number, further tokens ignored.  format 1, TSV:
 * a line is its fields between single tabs; an empty line is skipped; fewer than five fields make it MALFORMED (reason 2); else it
 * is a row: the last three fields are begin, end, number, the first is the file, and what lies between (tabs included) is the
 * header.  Its name is the first word of the header (between blanks; empty where it has none) -- but where the file field ends in
 * `.npz`, the piece of the file field behind its last '/' up to the first '.'.  A carriage return directly before the line feed
 * ends the line with it.
 * Rows, in file order, i = 0 .. rows - 1: d_begin[i], d_end[i], d_number[i] (int64), d_name_pos[i] / d_name_len[i] (the name as a
 * span of d_text), d_line[i] (from 1); TSV only, d_file_pos[i] / d_file_len[i] (the file field; both may be NULL for a table).
 * d_run_first[r], r = 0 .. runs - 1: the first row of run r, a maximal stretch of rows whose names (TSV: and file fields) are
 * byte-equal.  h_counts[6] (host): lines, rows, runs, the not-decided flag, the line (from 1) of the first malformed line or 0, its
 * reason.
 * NOT DECIDED: a byte outside 0x20..0x7e other than tab and line feed, a carriage return not directly before a line feed, or a
 * begin, end or number that is not 1..18 plain decimal digits (a sign, '_', a blank inside a TSV field, 19 digits).  Then
 * h_counts[3] = 1, no row is written and DGRP_OK is returned: the caller parses such a file on the host.  A MALFORMED line in a
 * file that is decided: h_counts[4] and [5] state the first, no row is written, DGRP_OK.  More rows than `cap`: DGRP_ENOMEM,
 * h_counts[1] = the capacity needed, no row written; n / 8 + 1 rows always suffice.  n = 0: zero counts.  Refused before any launch
 * with DGRP_EINVAL: NULL text with n > 0, n < 0, another format, a NULL output with cap > 0, NULL counts; with DGRP_ENOMEM: a
 * workspace (256-byte aligned) below dgrp_rows_parse_workspace_bytes(n).
 * The work split is dgrp_rm_parse's: DGRP_RM_TILE_BYTES per workgroup, a lane per 128 bytes and the lines that start there; a count
 * pass, two scans, a write pass, then the run flags, their scan and the run starts.  Integers only; the only atomics are the OR of
 * the flag and the min of the first malformed line's position: the same call gives the same bytes.  On the caller's stream; it
 * SYNCHRONISES that stream twice (counts, then runs; once where no row is written) and allocates nothing. */
int64_t dgrp_rows_parse_workspace_bytes(int64_t n);
int dgrp_rows_parse(const uint8_t *d_text, int64_t n, int format, int64_t *d_begin, int64_t *d_end, int64_t *d_number,
                    int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_file_pos, int32_t *d_file_len, int64_t *d_line,
                    int64_t *d_run_first, int64_t cap, int64_t *h_counts, void *d_work, int64_t work_bytes, void *stream);

/* ---- GFF3 read on the device (an addition, `compare` and `evaluate` with the format `gff3`).  THE GRAMMAR, stated
 * here once:
 * TEXT, LINES, END OF FEATURES.  The text is d_text[0..n), any alignment.  Lines end at LF; a CR directly before the LF belongs to
 * the line end.  E is the offset of the first line that is exactly `##FASTA` or that starts with '>', n where there is none: no byte
 * at or after E is read as a line (or raises the flag below), and E is reported.  An empty line is skipped; so is a line whose first
 * byte is '#'.
 * FIELDS.  Any other line is a feature line: fields between single tabs.  Fewer than nine fields make it MALFORMED (reason 3); the
 * ninth field runs to the line end, further tabs included.  Field 1 is the seqid: its span is the row's name, bytes as they stand
 * (not decoded here).  Fields 4 and 5 are start and end, each 1..18 plain decimal digits, 1-based and closed: begin = start - 1,
 * end = end, so start 0 gives begin -1, which the caller reports as a negative begin.
 * THE LABEL STRING.  key_len == 0: field 3, the type.  Otherwise field 9 is cut at every ';', a piece at its first '=' into tag and
 * value (a piece without '=' has no tag), and the first piece whose tag is byte-equal to d_key[0..key_len) gives the value; nothing
 * is trimmed or split at commas, and a key that is a proper prefix of a tag (`Name` against `Names=`) does not match.  The string
 * is compared DECODED: '%' followed by two hex digits of either case, both inside the string, stands for that byte; any other '%'
 * is itself.  Decoding happens during the comparison; nothing is written back.
 * THE NUMBER (int64).  d_names / d_name_off [nnames + 1] / d_name_number [nnames] (device): nnames alternatives
 * d_names[d_name_off[k] .. d_name_off[k + 1]) in ASCENDING byte order (memcmp, a proper prefix first; distinct), found by binary
 * search -- the rule is exact equality with the decoded label string.  The row's number is d_name_number[k] of that alternative; 0
 * where none is equal, where no piece has the key, and for an empty table.  A table that is not in that order gives numbers that
 * are not specified; the search stays inside it.
 * Rows, counts and runs are dgrp_rows_parse's for a table (no file spans): d_begin, d_end, d_number, d_name_pos / d_name_len,
 * d_line (from 1), d_run_first.  h_counts[7] (host): the lines in front of E, rows, runs, the not-decided flag, the line of the
 * first malformed line or 0, its reason, E.
 * NOT DECIDED (in front of E): a byte outside 0x20..0x7e other than tab and LF, a CR not directly before a LF, a start or end that
 * is not 1..18 plain digits.  Then h_counts[3] = 1, no row is written, DGRP_OK: the caller parses the file on the host.  MALFORMED
 * in a file that is decided: h_counts[4] and [5] state the first such line, no row is written, DGRP_OK.  More rows than `cap`:
 * DGRP_ENOMEM, h_counts[1] = the capacity needed, no row written.  The shortest feature line has 11 bytes (eight tabs, one digit
 * each for start and end, the LF), so n / 11 + 1 rows always suffice, and the at most 128 / 11 + 1 = 12 rows that start in a
 * lane's 128 bytes fit the uint8 the count pass keeps per lane.  n = 0: zero counts.  Refused before any launch with DGRP_EINVAL:
 * NULL text with n > 0, n < 0, nnames outside 0..4096, a NULL table pointer with nnames > 0, key_len outside 0..255, a NULL key with
 * key_len > 0, a NULL output with cap > 0, NULL counts, a workspace that is NULL or not 256-byte aligned; with DGRP_ENOMEM: a
 * workspace below dgrp_gff_parse_workspace_bytes(n).
 * The work split is dgrp_rows_parse's, with one kernel in front: a 64-bit atomicMin over the line starts that end the features
 * leaves E in the workspace; the count and write passes read it THERE (kernels of one stream are ordered, so no synchronisation is
 * spent on it) and walk d_text[0..E), which ends in a line feed.  Integers and bytes only; the only atomics are the OR of the flag
 * and the two minima: the same call gives the same bytes.  On the caller's stream; it SYNCHRONISES that stream twice (counts and
 * E, then runs; once where no row is written) and allocates nothing. */
int64_t dgrp_gff_parse_workspace_bytes(int64_t n);
int dgrp_gff_parse(const uint8_t *d_text, int64_t n, const uint8_t *d_names, const int64_t *d_name_off, const int32_t *d_name_number,
                   int nnames, const uint8_t *d_key, int key_len, int64_t *d_begin, int64_t *d_end, int64_t *d_number,
                   int64_t *d_name_pos, int32_t *d_name_len, int64_t *d_line, int64_t *d_run_first, int64_t cap, int64_t *h_counts,
                   void *d_work, int64_t work_bytes, void *stream);

/* ---- off-target (an addition, evaluate --offtarget): what the predicted repeats lie on.
 * dgrp_token_ids: dense ids for `rows` tokens given as spans of d_text [n] (device).  Token i is the bytes d_pos[i] .. + d_len[i],
 * and with d_len2[i] > 0 the logical string of those bytes, '/', and the bytes d_pos2[i] .. + d_len2[i]; a one-span and a two-span
 * spelling of one string are one token.  d_fid[i] (device int32) = the rank of token i among the DISTINCT tokens in ascending byte
 * order (memcmp; a proper prefix first), from 0.  h_counts[3] (host): F = the number of distinct tokens, the overflow flag, the
 * bytes of the F strings back to back.  h_names [names_cap] / h_name_off [DGRP_TOKEN_MAX + 1] (host): those strings in id order.
 * An open-addressing table of DGRP_TOKEN_SLOTS 64-bit words in the workspace, EMPTY or the row that claimed the slot (one
 * atomicCAS); a row that meets a taken slot compares its own bytes with the claimant's and takes the slot when they are equal, else
 * probes on: exact, the hash is only where the search starts.  Which row claims a slot depends on timing, the token the slot stands
 * for does not: the same call gives the same d_fid bytes.  More than DGRP_TOKEN_MAX distinct tokens: h_counts[1] = 1, no id and no
 * name is written, DGRP_OK (the caller numbers such a file on the host).  DGRP_EINVAL: a span that leaves the text (checked on the
 * device before a byte of it is read), NULL pointers with rows > 0; DGRP_ENOMEM: a workspace (256-byte aligned) below
 * dgrp_token_ids_workspace_bytes(rows, names_cap), or names of more than names_cap bytes (h_counts[2] tells the need).  It
 * SYNCHRONISES the stream three times: the count and the representative spans (one copy), the strings (one copy; the host sorts
 * them), and behind the kernel that writes d_fid.  rows == 0: zero counts, no device work. */
#define DGRP_TOKEN_SLOTS 65536
#define DGRP_TOKEN_MAX 16384
int64_t dgrp_token_ids_workspace_bytes(int64_t rows, int64_t names_cap);
int dgrp_token_ids(const uint8_t *d_text, int64_t n, int64_t rows, const int64_t *d_pos, const int32_t *d_len, const int64_t *d_pos2,
                   const int32_t *d_len2, int32_t *d_fid, uint8_t *h_names, int64_t names_cap, int64_t *h_name_off, int64_t *h_counts,
                   void *d_work, int64_t work_bytes, void *stream);
/* dgrp_paint_keys_batch: dgrp_paint_strata_batch (one body) with an arbitrary key per row: d_row_key[i] (device uint32) is the key
 * of row d_rows[i], whose own label is NOT read.  Every element of d_keys[0 .. h_off[nrec]) is written: 0xFFFFFFFF where no row
 * covers the base, else the smallest key among the rows that do.  DGRP_EINVAL before anything is written unless every row has
 * 0 <= start <= end and a key below 0xFFFFFFFF (one check kernel, one synchronisation).  Workspace: dgrp_eval_workspace_bytes.
 * dgrp_key_crosstab_batch: d_pred (int8) and d_keys (uint32, 4-byte aligned) are flat tracks of n bases, laid out as for
 * dgrp_confusion_matrix.  For every base, d_hist[p][k'] += 1 (device int64 [C][K], 8-byte aligned) with k' = key for key < K - 1 and
 * k' = K - 1 for 0xFFFFFFFF (K = 64 + F + 1).  Any other key, or p outside 0 .. C - 1, sets *d_bad (device int) and the base is not
 * counted; the call still returns DGRP_OK.  d_hist and *d_bad are zeroed on every call.  32-bit counters in LDS, sized so that none
 * can wrap, flushed with 64-bit atomic adds; where C * K counters exceed 160 KiB the cells are cut into groups of 40960 along
 * grid.y and every group reads every base: the bytes do not depend on the cut.  Stream-ordered: nothing synchronises.  DGRP_EINVAL
 * unless 1 <= C <= 64, 65 <= K <= 64 + DGRP_TOKEN_MAX + 1, 0 <= n < 2^40.
 * dgrp_row_key_classes_batch: rows, records, checks (labels 1..63), workspace and balancing by clipped length as for
 * dgrp_row_hits_batch, against a uint32 key track.  For row i with label L, d_cls[4 * i .. 4 * i + 4) (device int64) = the bases
 * of its clipped span with key == L; key < 64 and != L; 64 <= key < 0xFFFFFFFF; key == 0xFFFFFFFF.  Integer sums: the four add up
 * to the clipped length. */
int dgrp_paint_keys_batch(uint32_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                          const dgrp_segment *d_rows, const int64_t *h_row_off, const uint32_t *d_row_key, void *d_work,
                          int64_t work_bytes, void *stream);
int dgrp_key_crosstab_batch(const int8_t *d_pred, const uint32_t *d_keys, int64_t n, int C, int64_t K, int64_t *d_hist, int *d_bad,
                            void *stream);
int dgrp_row_key_classes_batch(const uint32_t *d_keys, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                               const dgrp_segment *d_rows, const int64_t *h_row_off, int64_t *d_cls, void *d_work, int64_t work_bytes,
                               void *stream);

/* ---- boundaries (an addition, evaluate --boundaries): how well a found element is delimited -- edge offsets and fragmentation.
 * dgrp_row_bounds_batch: records, track, rows, the row check (labels 1..127, one synchronisation, DGRP_EINVAL before anything is
 * written) and the balancing as for dgrp_row_hits_batch.  For row i with label L and clipped span [a, e) of a record of n bases from
 * coordinate o, with in(b) = "the track byte at coordinate b equals L":
 *   hits  = #{b in [a, e) : in(b)}                                    -- what dgrp_row_hits_batch gives
 *   runs  = #{b in [a, e) : in(b) and (b == a or !in(b - 1))}
 *   first / last = the smallest / largest b in [a, e) with in(b), in ORIGINAL coordinates; -1 when hits == 0
 *   lead  = the largest k <= min(W, a - o) with in(a - j) for every j = 1..k
 *   trail = the largest k <= min(W, o + n - e) with in(e - 1 + j) for every j = 1..k
 * and hits = runs = lead = trail = 0, first = last = -1 for an empty clipped span.  d_bounds[i] (8-byte aligned) is written for i in
 * [h_row_off[0], h_row_off[nrec]) and nowhere else.  0 <= W <= 4096, else DGRP_EINVAL.  One pass over the line of positions of the
 * WIDENED spans -- a row contributes min(W, a - o) + (e - a) + min(W, o + n - e) positions, 1 byte read per position, workgroups take
 * slices of 8192 positions -- between two one-lane-per-row kernels; no flank reads outside its record.  Integer adds, minima and
 * maxima: the same bytes on every run.  Workspace dgrp_row_bounds_workspace_bytes(nrec, rows), DGRP_ENOMEM below it.  After the row
 * check the entry is stream-ordered and allocates nothing.  nrec == 0 or no rows: no device work.
 * dgrp_bound_hist_batch: the rows and record tables of that call, its d_bounds, d_need (device int64 per row, read for i in
 * [h_row_off[0], h_row_off[nrec]) as dgrp_row_detect_batch reads it), 2 <= C <= 64 and the same W.  d_frag int64 [C][17], d_edge int64
 * [C][2][2W + 1], d_tally int64 [C][2] (8-byte aligned) and *d_bad (device int) are zeroed, then for every row with a non-empty
 * clipped span and label L: d_frag[L][min(runs, 16)] += 1; the row is FOUND when d_need[i] > 0 && hits >= d_need[i]; a found row adds
 * 1 to d_tally[L][0], has the offsets
 *   ds = first > a ? min(first - a, W) : -lead         de = last + 1 < e ? -min(e - 1 - last, W) : trail
 * (negative ds, positive de: the track's run sticks out beyond the row; +-W: W or more), adds 1 to d_edge[L][0][ds + W] unless the
 * record clipped its start (start < o), 1 to d_edge[L][1][de + W] unless the record clipped its end (end > o + n), and 1 to
 * d_tally[L][1] when neither side is clipped and ds == de == 0.  A label outside 0..C-1 (or bounds taken with a larger W) sets
 * *d_bad and the row is not counted; the call still returns DGRP_OK.  One lane per row, 32-bit counters in LDS (the edge offsets
 * where C * 2 * (2W + 1) of them fit 64 KiB beside the others, else added to d_edge directly), flushed with 64-bit atomic adds.
 * Stream-ordered: nothing synchronises, no row is checked.  Workspace dgrp_bound_hist_workspace_bytes(nrec) (the record tables),
 * DGRP_ENOMEM below it.  No rows: the outputs are zeroed, nothing else runs. */
typedef struct { int64_t hits, runs, first, last; int32_t lead, trail; } dgrp_row_bound;   /* 40 bytes */
int64_t dgrp_row_bounds_workspace_bytes(int64_t nrec, int64_t nrows);
int dgrp_row_bounds_batch(const int8_t *d_labels, int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin,
                          const dgrp_segment *d_rows, const int64_t *h_row_off, int W, dgrp_row_bound *d_bounds, void *d_work,
                          int64_t work_bytes, void *stream);
int64_t dgrp_bound_hist_workspace_bytes(int64_t nrec);
int dgrp_bound_hist_batch(int64_t nrec, const int64_t *h_off, const int64_t *h_len, const int64_t *h_origin, const dgrp_segment *d_rows,
                          const int64_t *h_row_off, const dgrp_row_bound *d_bounds, const int64_t *d_need, int C, int W, int64_t *d_frag,
                          int64_t *d_edge, int64_t *d_tally, int *d_bad, void *d_work, int64_t work_bytes, void *stream);

/* ---- instrumentation (bench.py's roofline figure; no counterpart in the reference, no effect on results).
 * While enabled for the CALLING HOST THREAD, every launch of a recurrent forward kernel (GRU / LSTM, fused or split) that this
 * thread makes through any entry point above is bracketed by two HIP events on the launch's stream.  dgrp_kernel_timer_read waits
 * for the recorded events, returns the summed device time in milliseconds, the number of launches and the windows they covered,
 * and forgets them; enabling again also starts from an empty list. */
int dgrp_kernel_timer_enable(int on);
int dgrp_kernel_timer_read(double *h_ms, int64_t *h_launches, int64_t *h_windows);

#ifdef __cplusplus
}
#endif
#endif /* DEEPGRP_HIP_H_ */
