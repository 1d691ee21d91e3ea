/*
 * b64x.h -- C ABI of the MI355X (gfx950) base64 engine.
 *
 * This is the thin shim between host code (the bytestream_1 stages in
 * include/base64encoder.h / base64decoder.h, Python via ctypes, any FFI)
 * and the hand-written HIP kernels in async_amd/csrc/b64x_kernels.hip.
 * Only plain pointers, sizes and PODs cross it; no HIP or torch types.
 *
 * What each entry point replaces in the reference (all C, CPU only):
 *
 *   b64x_encode_dev / _strided / _batch
 *       the per-byte bit-accumulator loop of do_read() + finalize(),
 *       /root/reference/src/base64encoder.c:61-142, applied to a whole
 *       device-resident buffer (or a batch of independent buffers -- one
 *       encoder object per buffer in the reference).
 *   b64x_decode_dev / _strided / _batch
 *       the per-character loop of decoder_read() with map(),
 *       /root/reference/src/base64decoder.c:38-80, including its
 *       leniency (non-alphabet bytes skipped, bits carried across '=',
 *       trailing partial bits dropped).
 *   b64x_session_*
 *       the host-memory leg of the bytestream_1 stages: pinned staging,
 *       H2D, kernel, D2H.
 *
 * Error convention: 0 on success or a negative errno value (-EINVAL bad
 * argument, -ENOMEM allocation, -ENODEV no usable GPU, -EIO any other
 * HIP failure).  Nothing here aborts.
 *
 * All device pointers are HIP device (or host-pinned-mapped) pointers.
 * `stream` is a hipStream_t passed as void * (NULL = the null stream).
 * Device-side launches are asynchronous and capture-safe (no allocation
 * or synchronisation inside) unless the comment says otherwise.  A call
 * being captured into a graph does not reuse a line model held from earlier
 * calls (it captures the probe or prep too); the junk hint's pick of path is
 * replayed as made at capture -- exact either way, only the speed differs.
 */
/*
 * Process-wide state a decode call reads and writes.  None of it decides a
 * byte of output: every path below is exact for any input, and the state only
 * picks which path runs (b64x_diag_paths counts the picks).
 *
 *   library workspaces   at most 8, one per (device, stream), for calls with
 *                        d_workspace NULL and for b64x_decode_strided's rows
 *                        with room.  Read and written by those calls: scratch
 *                        (left zeroed), the probe's line model with the length
 *                        it was made for, a row batch's model and the shape it
 *                        was made for.  Guarded by a mutex; an entry is pinned
 *                        while a call enqueues on it.
 *   held models          64 entries keyed by a hash of the workspace address:
 *                        {workspace, length of its last probe}, plus a pinned
 *                        "probe again" flag each.  Read by every automatic
 *                        b64x_decode_dev of <= 2^31 characters (not
 *                        EXPECT_JUNK): a call of the same length on the same
 *                        workspace with the flag down skips the probe.
 *                        Written by every probe launch (host) and by
 *                        k_decode_suffix, which raises the flag whenever it
 *                        finds anything to decode past the line pass.  Any
 *                        model is exact (k_decode_lines checks every slot and
 *                        the model's length); a wrong one only costs speed.
 *   probe hints          64 pinned entries keyed by a hash of (workspace,
 *                        input address, length): "the last probe of this key
 *                        cut the model near the start".  Read (without a
 *                        sync) by every automatic decode, which then takes the
 *                        probe + single exact pass; written by every probe on
 *                        the device.  A stale or torn hint only picks the
 *                        slower path; new content at the same address and
 *                        length is decoded exactly either way.
 *   row-model staleness  one pinned flag per library workspace, raised by
 *                        k_rows_finish when a batch's first row failed its
 *                        model; read by the next b64x_decode_strided of the
 *                        same shape on that workspace, which then probes.
 *   sequence numbers     one counter, drawn by every decode call and batch
 *                        (b64x_dec_result.seq).
 *
 * A call being captured into a graph reads no held model or row model (it
 * captures the probe or prep), and never allocates or takes over a library
 * workspace.  The hint's pick is recorded in the capture as made.
 */

#ifndef ASYNC_AMD_B64X_H
#define ASYNC_AMD_B64X_H

#include <stdbool.h>
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define B64X_ABI_VERSION 7

/* Alphabet descriptor.  (char) -1 selects the reference's defaults,
 * exactly like base64_encode()/base64_decode() (ref
 * src/base64encoder.c:40-43, src/base64decoder.c:31-32).  `pad` and
 * `padchar` are ignored by the lenient decoder, which has no pad parameter
 * (b64x_decode_strict_* honour them). */
typedef struct b64x_alphabet {
    char pos62;
    char pos63;
    char padchar;
    bool pad;
} b64x_alphabet;

/* Per-call decode result, written by the device.  A record names the call
 * that wrote it: `nchars` and `flags` echo the call's arguments and `seq` is
 * a nonzero number the library draws for every decode call (or batch), so
 * a record left over from an earlier call, or a zero-filled one, is never
 * taken for this call's (b64x_session_decode_result, b64x_lane_decode_check). */
typedef struct b64x_dec_result {
    uint64_t out_len;  /* bytes written to the output */
    uint64_t valid;    /* alphabet characters seen (V) */
    uint32_t tail_n;   /* V mod 4 */
    uint8_t tail[4];   /* the last tail_n sextet values (0..63); the rest 0 */
    uint64_t nchars;   /* characters this decode covered */
    uint32_t seq;      /* the call's sequence number, never 0 */
    uint32_t flags;    /* the call's B64X_DEC_HOLD_TAIL bit */
} b64x_dec_result;

/* Decode flags. */
#define B64X_DEC_HOLD_TAIL 1u /* emit only whole 4-char groups (3 bytes
                                 each); the V mod 4 trailing sextets are
                                 reported in b64x_dec_result.tail and
                                 produce no output.  Used by the streaming
                                 stage, which carries them to its next
                                 call. */
#define B64X_DEC_EXPECT_JUNK 2u /* a hint that the input holds non-alphabet
                                   bytes throughout (MIME line breaks):
                                   decode in one pass (counts, look-back,
                                   exact decode) instead of the optimistic
                                   pass that clean input takes.  Same
                                   result either way. */

/* ---- sizes ------------------------------------------------------------ */

/* Characters produced for n input bytes: 4*ceil(n/3) with pad,
 * ceil(4n/3) without. */
uint64_t b64x_encoded_len(uint64_t n, bool pad);
/* Output capacity the decoder needs for n input characters:
 * 3*ceil(n/4).  Bytes beyond b64x_dec_result.out_len are unspecified
 * (the reference likewise treats the caller's whole buffer as scratch,
 * src/base64decoder.c:58). */
uint64_t b64x_decoded_cap(uint64_t nchars);
/* Device workspace bytes b64x_decode_dev() needs for nchars. */
uint64_t b64x_decode_workspace_size(uint64_t nchars);

/* ---- one device-resident buffer ----------------------------------------- */

/* Encode n bytes at d_in into b64x_encoded_len(n, abc->pad) characters at
 * d_out.  Any alignment is accepted; 4-byte aligned d_in and 16-byte
 * aligned d_out take the fast path. */
int b64x_encode_dev(const void *d_in, uint64_t n, void *d_out,
                    const b64x_alphabet *abc, void *stream);

/* Decode nchars characters at d_in into d_out (capacity
 * b64x_decoded_cap(nchars)); *d_res (device memory) receives the result.
 * d_workspace: b64x_decode_workspace_size(nchars) bytes of device memory,
 * zero-filled before its first use (each call leaves it ready for the
 * next, holding the line model of its last probe: a call of the same length
 * may reuse it and skip the probe; one workspace per stream), or NULL to use
 * a library-owned one
 * per (device, stream).  The library keeps at most 8 such workspaces
 * (about 14 MiB of HBM each), allocated on first need and never freed: a
 * call on a stream without one takes an idle one (its stream made to wait
 * on the device for the workspace's last use), or -EBUSY if all eight are
 * in use by calls being enqueued right then.  A stream being captured into
 * a graph that holds no library workspace yet also gets -EBUSY (allocating
 * or rebinding one cannot be captured): decode on it once outside the
 * capture, or pass d_workspace.  A workspace stays with its stream until
 * b64x_release_stream() or until another stream takes it over; no event is
 * recorded per call. */
int b64x_decode_dev(const void *d_in, uint64_t nchars, void *d_out,
                    b64x_dec_result *d_res, const b64x_alphabet *abc,
                    unsigned flags, void *d_workspace, void *stream);
/* b64x_decode_dev, also returning in *seq (may be NULL) the sequence number
 * the call drew: the `seq` its record holds once it has landed.  A caller
 * that copies the record back (from any stream) checks it with
 * b64x_result_check() and so never takes a stale, zero-filled or partly
 * written record for this call's. */
int b64x_decode_dev_seq(const void *d_in, uint64_t nchars, void *d_out,
                        b64x_dec_result *d_res, const b64x_alphabet *abc,
                        unsigned flags, void *d_workspace, void *stream, uint32_t *seq);
/* 0 if *res (host memory) is the landed, self-consistent record of the
 * decode of `nchars` characters with `flags` that drew `seq` (the rules of
 * b64x_session_decode_result), -EAGAIN if it is not (yet). */
int b64x_result_check(const b64x_dec_result *res, uint64_t nchars, unsigned flags,
                      uint32_t seq);
/* Unbind the library-owned decode workspace of `stream` on the current
 * device, if it has one, so another stream can take it.  REQUIRED before
 * destroying a stream that decoded with d_workspace == NULL: the workspace
 * stays bound to the stream's handle, and a later call on another stream
 * that takes it over records an event on that handle (and asks whether it
 * is being captured) -- on a destroyed stream that is a dangling handle.
 * Released here, the event is recorded while the stream is still alive.
 * The NULL stream may hold a workspace like any other. */
void b64x_release_stream(void *stream);

/* ---- batches of independent buffers ----------------------------------- */

/* nbuf buffers of `len` bytes at d_in + i*in_stride; buffer i's
 * b64x_encoded_len(len, pad) characters go to d_out + i*out_stride. */
int b64x_encode_strided(const void *d_in, uint64_t in_stride, uint64_t len,
                        uint32_t nbuf, void *d_out, uint64_t out_stride,
                        const b64x_alphabet *abc, void *stream);

/* nbuf buffers of `len` characters at d_in + i*in_stride, decoded to
 * d_out + i*out_stride (capacity b64x_decoded_cap(len) each);
 * d_outlen[i] (device) receives buffer i's byte count.  Rows with room
 * (out_stride >= 12*ceil(len/16)) use the stream's library workspace (as
 * b64x_decode_dev with d_workspace NULL) to hold the batch's line model;
 * when none can be had (all pinned, or a capture on a stream holding none)
 * the batch takes the general path, same bytes.  In a row with room the
 * bytes from d_outlen[i] up to min(out_stride, 12*ceil(len/16)) are scratch
 * (whole 12-byte slots are stored, and slack up to the stride is filled);
 * on the general path those up to b64x_decoded_cap(len) are; nothing else
 * outside a buffer's d_outlen[i] bytes is written. */
int b64x_decode_strided(const void *d_in, uint64_t in_stride, uint64_t len,
                        uint32_t nbuf, void *d_out, uint64_t out_stride,
                        uint64_t *d_outlen, const b64x_alphabet *abc,
                        void *stream);

/* Ragged batch: buffer i is d_in[d_in_off[i] .. d_in_off[i+1]) (nbuf+1
 * monotone offsets, device memory) and goes to d_out + d_out_off[i]. */
int b64x_encode_batch(const void *d_in, const uint64_t *d_in_off,
                      uint32_t nbuf, void *d_out, const uint64_t *d_out_off,
                      const b64x_alphabet *abc, void *stream);
int b64x_decode_batch(const void *d_in, const uint64_t *d_in_off,
                      uint32_t nbuf, void *d_out, const uint64_t *d_out_off,
                      uint64_t *d_outlen, const b64x_alphabet *abc,
                      void *stream);

/* ---- line-wrapped encode (MIME 76/CRLF, PEM 64/LF) --------------------- */

/* The shape of line-wrapped base64 text: lines of line_len characters, each
 * followed by the separator.  line_len must be a multiple of 4 (>= 4), so
 * that line k is the plain encoding of input bytes [3k*line_len/4,
 * 3(k+1)*line_len/4) and every line starts on a 3-byte group. */
typedef struct b64x_lines {
    uint32_t line_len;   /* L: alphabet/pad characters per line; a multiple of 4, >= 4 */
    uint32_t sep_len;    /* s: 1..4 */
    uint8_t  sep[4];     /* the separator bytes; the first sep_len are used */
    uint32_t flags;      /* B64X_LINES_TRAILING */
} b64x_lines;
#define B64X_LINES_TRAILING 1u  /* also write the separator after the last line */

/* Bytes b64x_encode_lines_dev() writes for n input bytes: with E =
 * b64x_encoded_len(n, pad), E + s*(ceil(E/L) - (trailing ? 0 : 1)) for
 * E > 0, and 0 for E == 0 (or an invalid fmt). */
uint64_t b64x_encoded_lines_len(uint64_t n, bool pad, const b64x_lines *fmt);

/* Encode n bytes at d_in as line-wrapped text at d_out: the characters
 * b64x_encode_dev() writes for the same input and alphabet, cut into
 * ceil(E/L) lines of L characters (the last may be shorter), the separator
 * after every line but the last and, with B64X_LINES_TRAILING, after the
 * last one too; nothing for n == 0.  Exact: no model, no hint.
 * L = 76, "\n", trailing is Python's base64.encodebytes; L = 76, "\r\n" is
 * RFC 2045; L = 64, "\n", trailing is a PEM body.
 * -EINVAL: fmt NULL, L == 0 or not a multiple of 4, s outside 1..4, unknown
 * flag bits, or a separator byte that is an alphabet character under abc
 * (the 62 alphanumerics and the effective pos62/pos63: the text would not
 * decode back).  Checked in this order: n == 0 returns 0, NULL buffers
 * -EINVAL, the format, then -ENODEV without a gfx950 device (no CPU path).
 * Input and output must not overlap.  Any alignment is accepted; 4-byte
 * aligned d_in with 16-byte aligned d_out is the fast path.  No 32-bit limit
 * on n.  The launch is asynchronous and capture-safe: the format travels as
 * kernel arguments, nothing is allocated or synchronised. */
int b64x_encode_lines_dev(const void *d_in, uint64_t n, void *d_out,
                          const b64x_alphabet *abc, const b64x_lines *fmt, void *stream);

/* nbuf rows of `len` bytes at d_in + i*in_stride, each wrapped on its own
 * into d_out + i*out_stride; every row gets b64x_encoded_lines_len(len, pad,
 * fmt) bytes.  -EINVAL also for out_stride below that length or in_stride <
 * len.  Rows at 4-byte aligned addresses (both sides) are the fast shape. */
int b64x_encode_lines_strided(const void *d_in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
                              void *d_out, uint64_t out_stride,
                              const b64x_alphabet *abc, const b64x_lines *fmt, void *stream);

/* ---- strict decode with first-error position --------------------------- */

/* b64x_decode_strict_* accept exactly the texts the encoders above write
 * under the same alphabet and line format -- strict(t) accepts <=> t ==
 * encode[_lines](decode(t)) -- decode them, and otherwise report the kind and
 * the byte offset of the first offence.  Unlike the lenient decoder they read
 * `abc` as the encoder does: (char) -1 gives the defaults, and `pad` /
 * `padchar` are honoured.
 *
 * The result is, for any input, what this scalar procedure returns:
 *  1. Length, from nchars, fmt and pad alone.  Plain: E = nchars.  Wrapped
 *     (P = L + s): m = nchars (trailing) or nchars + s, (k, r) = divmod(m, P);
 *     r == 0: E = kL; r > s: E = kL + r - s; 0 < r <= s: no E; nchars == 0:
 *     E = 0.  There is no valid E either if b64x_encoded_lines_len's formula
 *     for E does not give nchars back, if pad and E mod 4 != 0, or if not pad
 *     and E mod 4 == 1.  No E: {LENGTH, err_pos = nchars}, nothing is read.
 *  2. Positions.  Character e stands at offset e (plain) or floor(e/L) P +
 *     e mod L.  The separator follows every line, a short last one included;
 *     it follows the very last line only with B64X_LINES_TRAILING.
 *  3. Pads.  With pad, npad = 0 unless character E-1 is the pad character;
 *     then 2 if character E-2 is too, else 1.  Without pad, 0.  D = E - npad.
 *  4. Offences.  A separator byte != sep[j] is SEP.  A character e < D that
 *     is the pad character (with pad) is PAD, else one outside the 64 is
 *     CHAR.  Character D-1, with D mod 4 in {2, 3}, whose sextet has any of
 *     its low 4 / 2 bits set is BITS.  A byte has at most one kind; the
 *     record holds the kind and offset of the offence at the lowest offset,
 *     however many there are.
 *  5. No offence: out_len = 3 floor(D/4) + (0, -, 1, 2)[D mod 4], and the
 *     bytes are those of the D sextets. */
#define B64X_STRICT_OK      0u
#define B64X_STRICT_CHAR    1u  /* a byte at a character position that is neither in the alphabet nor the pad character */
#define B64X_STRICT_SEP     2u  /* a byte at a separator position that is not that separator byte */
#define B64X_STRICT_PAD     3u  /* the pad character where no pad may stand */
#define B64X_STRICT_BITS    4u  /* the last data character carries nonzero unused low bits */
#define B64X_STRICT_LENGTH  5u  /* no encoder output has this length; err_pos == nchars */

typedef struct b64x_strict_result {
    uint64_t out_len;   /* bytes decoded; 0 when err != 0 */
    uint64_t err_pos;   /* offset in the text of the first offence; 0 when err == 0 */
    uint32_t err;       /* B64X_STRICT_* */
    uint32_t reserved;  /* 0 */
} b64x_strict_result;

/* Output capacity of a strict decode of nchars bytes of text: 3*ceil(E/4)
 * for the E characters a text of that length holds (step 1 without the pad
 * rules; a length no text has counts the characters of its whole lines).
 * fmt NULL: plain.  Never more than b64x_decoded_cap(nchars); 0 for a fmt
 * with line_len == 0, sep_len outside 1..4 or line_len + sep_len past
 * 2^32 - 1 (no call accepts such a fmt). */
uint64_t b64x_strict_decoded_cap(uint64_t nchars, const b64x_lines *fmt);

/* Strictly decode the nchars bytes at d_in (fmt NULL: plain text) into d_out
 * (capacity b64x_strict_decoded_cap(nchars, fmt)); *d_res (device memory,
 * 8-byte aligned) receives the record.  The call writes the whole record
 * itself (the caller need not zero it), nothing outside [d_out, d_out + cap)
 * and the record, and reads nothing outside [d_in, d_in + nchars).  With
 * err != 0 the output bytes are unspecified.  nchars == 0 is a valid text
 * (out_len 0) and still writes its record.
 * -EINVAL: a NULL buffer or record (or a record not 8-byte aligned); a fmt
 * b64x_encode_lines_dev would refuse (the same rules in the same order);
 * pos62 == pos63; an alphanumeric pos62 or pos63; pad set and padchar one of
 * the 64 alphabet characters.  Then -ENODEV without a gfx950 device.
 * Asynchronous, capture-safe and exact: no allocation, no synchronisation, no
 * workspace, no library state, no hint (a memset node, the decode kernel and
 * a one-thread-per-row kernel that gives the record its final form).  Any
 * alignment is accepted; 4-byte aligned d_in and d_out with L >= 16 is the
 * fast path.  No 32-bit limit on nchars. */
int b64x_decode_strict_dev(const void *d_in, uint64_t nchars, void *d_out,
                           b64x_strict_result *d_res, const b64x_alphabet *abc,
                           const b64x_lines *fmt /* NULL: plain */, void *stream);

/* nbuf rows of `len` bytes of text at d_in + i*in_stride, each decoded on its
 * own into d_out + i*out_stride, its record in d_res[i] (err_pos is an offset
 * in the row).  -EINVAL also for in_stride < len or out_stride below
 * b64x_strict_decoded_cap(len, fmt).  Rows at 4-byte aligned addresses (both
 * sides) are the fast shape. */
int b64x_decode_strict_strided(const void *d_in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
                               void *d_out, uint64_t out_stride, b64x_strict_result *d_res /* nbuf */,
                               const b64x_alphabet *abc, const b64x_lines *fmt, void *stream);

/* ---- ragged batches of the two calls above ----------------------------- */

/* Both calls address their buffers as b64x_encode_batch does: buffer i is
 * d_in[d_in_off[i] .. d_in_off[i+1]) (nbuf + 1 monotone offsets, device
 * memory) and its output starts at d_out + d_out_off[i] (nbuf entries).  The
 * lengths are read on the device when the kernel runs: the grid and every
 * kernel argument depend on nbuf, abc and fmt only, so a call captured into a
 * graph can be replayed on batches of other lengths by rewriting the offset
 * arrays (the one-buffer and strided calls bake the length into their kernel
 * arguments).  Asynchronous, exact and capture-safe: no allocation, no
 * synchronisation, no workspace, no library state, no hint.
 * Any alignment of any buffer is accepted, mixed within one batch; a buffer
 * whose input and output addresses are both 4-byte aligned takes the fast
 * path (with L >= 16), the others are written bytewise.  No 32-bit limit on a
 * buffer's length -- but one wave walks one buffer, so a buffer of hundreds
 * of MiB, exact as it is, runs at one wave's rate (the kernels balance a
 * batch over buffers, not over the bytes of one): such a buffer belongs on
 * the one-buffer calls, as with b64x_encode_batch's one block per buffer --
 * or in a batch of the wide calls below, b64x_encode_batch_wide and
 * b64x_decode_strict_batch_wide. */

/* Buffer i wrapped on its own: byte for byte what b64x_encode_lines_dev()
 * writes for it under the same abc and fmt, b64x_encoded_lines_len(len_i,
 * pad, fmt) bytes; nothing for an empty buffer.  Nothing is written outside
 * those ranges, and nothing outside buffer i is read for its text.
 * Checked in this order: nbuf == 0 returns 0, NULL pointers -EINVAL, the
 * format rules of b64x_encode_lines_dev (fmt NULL is -EINVAL here: plain is
 * b64x_encode_batch), then -ENODEV. */
int b64x_encode_lines_batch(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                            void *d_out, const uint64_t *d_out_off,
                            const b64x_alphabet *abc, const b64x_lines *fmt, void *stream);

/* Text i strictly decoded on its own into d_out + d_out_off[i] (capacity
 * b64x_strict_decoded_cap(len_i, fmt)); d_res[i] is exactly the record the
 * scalar procedure above gives for text i alone, err_pos an offset inside the
 * buffer: {LENGTH, err_pos = len_i} where no encoder output has that length
 * (decided per buffer, on the device), {0, 0, OK} for an empty text.  The
 * call writes every record whole (the caller need not zero them), nothing
 * outside [d_out_off[i], d_out_off[i] + cap_i) and the records, and reads
 * nothing outside buffer i.  One kernel: a wave owns its buffer alone and
 * keeps the lowest offence to itself, so there is no memset node, no global
 * atomic and no record kernel.
 * Checked in this order: nbuf == 0 returns 0, NULL pointers (or a record array
 * not 8-byte aligned) -EINVAL, the format and alphabet rules of
 * b64x_decode_strict_dev, then -ENODEV. */
int b64x_decode_strict_batch(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                             void *d_out, const uint64_t *d_out_off,
                             b64x_strict_result *d_res /* nbuf */,
                             const b64x_alphabet *abc, const b64x_lines *fmt /* NULL: plain */,
                             void *stream);

/* The ragged encode balanced over the batch's bytes, not over its buffers:
 * an 8 MiB buffer among 4 KiB ones is spread over the device like the rest,
 * so the host need not look at the lengths to route the large ones to the
 * one-buffer calls.  Added within ABI 7 (a symbol only).
 * Buffers are addressed exactly as in b64x_encode_batch (d_in_off[0] may be
 * nonzero; an empty buffer writes nothing).  With fmt NULL buffer i gets byte
 * for byte what b64x_encode_batch writes for it, otherwise what
 * b64x_encode_lines_batch writes under the same abc and fmt; nothing is
 * written outside [d_out_off[i], d_out_off[i] + len_out_i).  Nothing is read
 * outside the arena [d_in + d_in_off[0], d_in + d_in_off[nbuf]) and the two
 * offset arrays, and the dword loads of a buffer's fast path stay inside that
 * buffer.
 * total_hint is the only length the host sees: it sizes the grid
 * (ceil(total_hint / 48 KiB) blocks, between 1 and 8 per CU) and nothing
 * else.  0 means "unknown: fill the device".  The result is exact for any
 * value, too small, too large or 0: each wave reads the arena's size on the
 * device and takes an equal span of it (at least 12 KiB), finds the span's
 * buffers by a binary search over d_in_off, and every 16-byte output block
 * of every buffer has exactly one owning span.  The grid and every kernel
 * argument depend on nbuf, total_hint, abc, fmt and the device alone: a
 * captured call replays on other offsets.
 * One launch: no workspace, no allocation, no synchronisation, no atomic, no
 * library state.  Any alignment of any buffer is accepted, mixed within a
 * batch (both addresses 4-byte aligned, and L >= 16 when wrapped, is a
 * buffer's fast path); no 32-bit limit on a buffer or on the arena.
 * It pays a search per wave: batches of many small buffers only are served
 * better by b64x_encode_batch / b64x_encode_lines_batch (README.md has the
 * measured crossing).
 * Checked in this order: nbuf == 0 returns 0, NULL pointers -EINVAL, with
 * fmt the format rules of b64x_encode_lines_dev, then -ENODEV. */
int b64x_encode_batch_wide(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                           uint64_t total_hint,
                           void *d_out, const uint64_t *d_out_off,
                           const b64x_alphabet *abc,
                           const b64x_lines *fmt /* NULL: plain */, void *stream);

/* The ragged strict decode balanced over the batch's bytes, not over its
 * texts: the decode and check of what b64x_encode_batch_wide writes, an 8 MiB
 * text among 4 KiB ones spread over the device like the rest.  Added within
 * ABI 7 (a symbol only).
 * Texts are addressed exactly as in b64x_decode_strict_batch (d_in_off[0] may
 * be nonzero): text i is d_in[d_in_off[i] .. d_in_off[i+1]), its bytes go to
 * d_out + d_out_off[i] (capacity b64x_strict_decoded_cap(len_i, fmt)), its
 * record to d_res[i].  For every i, d_res[i] is exactly the record the scalar
 * procedure above ("strict decode with first-error position") gives for text
 * i alone: {0, len_i, LENGTH} where no encoder output has that length
 * (decided per text, on the device; nothing of such a text is read),
 * {0, 0, OK} for an empty text.  Every record is written whole: the caller
 * prepares nothing.  An accepted text's bytes are byte for byte those of
 * b64x_decode_strict_batch; with err != 0 the text's output bytes are
 * unspecified but stay inside its capacity.  Nothing is written outside the
 * capacities and the records; nothing is read outside the arena
 * [d_in + d_in_off[0], d_in + d_in_off[nbuf]) and the two offset arrays, and
 * the dword windows of a text's fast path stay inside that text.
 * total_hint works as in b64x_encode_batch_wide: the only length the host
 * sees, it sizes the grid (ceil(total_hint / 64 KiB) blocks, between 1 and 8
 * per CU) and nothing else; 0 means "unknown: fill the device".  The result
 * is exact for any value: each wave reads the arena's size on the device and
 * takes an equal span of it (at least 16 KiB of text), finds the span's texts
 * by a binary search over d_in_off, and every 16-character lane of every text
 * belongs to the one span that holds its first character.  The grid and every
 * kernel argument depend on nbuf, total_hint, abc, fmt and the device alone:
 * a captured call replays on other offsets and contents.
 * Three graph nodes whatever the sizes, after b64x_decode_strict_dev: a
 * one-thread-per-text kernel that sets the 24 nbuf record bytes to ones (a
 * kernel, not a memset node: a captured memset node did not keep its bytes
 * from the second replay of a graph on), the decode kernel (a lane that finds
 * an offence lowers the text's key with one 64-bit atomic; good text performs
 * none) and a one-thread-per-text kernel that gives each record its final
 * form.  No workspace, no allocation, no synchronisation, no library state.
 * Any alignment of any text is accepted, mixed within a batch (both addresses
 * 4-byte aligned, and L >= 16 when wrapped, is a text's fast path); no 32-bit
 * limit on a text or on the arena.
 * It pays a search per wave and two record kernels: batches of many
 * texts that are all below 16 KiB are served better by
 * b64x_decode_strict_batch, a batch that holds texts from 32 KiB up by this
 * call (README.md has the measured crossing).
 * Checked in this order: nbuf == 0 returns 0, NULL pointers (or a record array
 * not 8-byte aligned) -EINVAL, with fmt the format rules of
 * b64x_decode_strict_dev, then its alphabet rules, then -ENODEV. */
int b64x_decode_strict_batch_wide(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                                  uint64_t total_hint,
                                  void *d_out, const uint64_t *d_out_off,
                                  b64x_strict_result *d_res /* nbuf */,
                                  const b64x_alphabet *abc,
                                  const b64x_lines *fmt /* NULL: plain */, void *stream);

/* ---- strict decode that skips line breaks ------------------------------ */

/* What `base64 -d`, a PEM reader or a mail library does lies between the
 * lenient decoder (every stranger skipped, nothing reported) and
 * b64x_decode_strict_* (one exact line format): a small, named set of bytes
 * -- CR and LF, perhaps space and tab -- is ignored wherever it stands,
 * anything else is refused, and the caller learns where the first offence is.
 * Added within ABI 7 (symbols only).
 *
 * `abc` is read as the strict decoder reads it ((char) -1 gives the
 * defaults; pad and padchar are honoured).  The record is b64x_strict_result;
 * B64X_STRICT_SEP is never reported.  The result for any text t[0..n) is what
 * this scalar procedure returns:
 *  1. Kept bytes.  u is the bytes of t that are not in the skip set, in
 *     order; kept byte e stands at offset o(e) of t.  E = |u|.
 *  2. Pads: step 3 of the strict procedure on u.  With pad, npad = 0 unless
 *     u[E-1] is the pad character; then 2 if u[E-2] is too, else 1.  Without
 *     pad, 0.  D = E - npad.  Skipped bytes may stand between the pads and
 *     after them.
 *  3. Offences at a byte.  A kept byte e < D that is the pad character (with
 *     pad) is PAD, else one outside the 64 is CHAR.  The record holds the
 *     kind and the offset o(e) of the offence at the lowest offset.  Unlike
 *     the strict calls, these come before LENGTH: the text has to be read to
 *     know E anyway, and the caller wants the position of the junk byte.
 *  4. Length.  No offence so far: {LENGTH, err_pos = n} if pad and
 *     E mod 4 != 0, or not pad and E mod 4 == 1.
 *  5. Unused bits.  None so far: BITS at o(D-1), as in strict step 4.
 *  6. Accepted: out_len = 3 floor(D/4) + (0, -, 1, 2)[D mod 4] and the bytes
 *     are those of the D sextets.  E == 0 (n == 0, or skipped bytes only) is
 *     accepted with out_len 0 and still writes the record.  With an offence,
 *     out_len = 0 and the output bytes are unspecified.
 * Consequence: the call accepts t if and only if b64x_decode_strict_dev(u,
 * plain) accepts u, and then with the same bytes.
 *
 * The bytes come from the lenient decoder on the caller's workspace: a
 * decoding call enqueues b64x_decode_dev (the batch: b64x_decode_batch) on
 * the same text, whose output for an accepted text is by definition these
 * bytes.  The verdict is a read-only pass of its own over the text and a
 * finish step; with d_out NULL only those run (validate only: the text is
 * read once and nothing but the record and the workspace head is written). */
typedef struct b64x_skip {
    uint32_t n;        /* 0..8 */
    uint8_t bytes[8];  /* the first n are skipped; duplicates are fine */
} b64x_skip;           /* NULL: {2, "\r\n"} */

/* Device workspace bytes of b64x_decode_strict_skip_dev: a fixed head (a
 * b64x_dec_result for the lenient decoder and a slot per block of the
 * checking pass), then, unless validate_only, b64x_decode_workspace_size(
 * nchars) bytes for the lenient decoder. */
uint64_t b64x_strict_skip_workspace_size(uint64_t nchars, bool validate_only);

/* Judge the nchars bytes at d_in as above and, with d_out not NULL, decode
 * them into d_out (capacity b64x_decoded_cap(nchars)); *d_res (device memory,
 * 8-byte aligned) receives the record, written whole by the call.
 * d_workspace: b64x_strict_skip_workspace_size(nchars, d_out == NULL) bytes
 * of device memory, 8-byte aligned.  The head needs no preparation.  The part
 * behind it is b64x_decode_dev's d_workspace and inherits its rules: zero
 * before its first use, one per stream; the lenient decoder's held models and
 * hints work on it as they do there, and none of them decides a byte.
 * Checked in this order: a NULL d_in, d_res or d_workspace (or a record or
 * workspace not 8-byte aligned) is -EINVAL -- d_out may be NULL, and
 * nchars == 0 still wants a d_in; a skip set with n > 8, or with a byte that
 * is one of the 64 characters under abc or (with pad) the pad character, is
 * -EINVAL; the alphabet rules of b64x_decode_strict_dev; then -ENODEV without
 * a gfx950 device.
 * Asynchronous and capture-safe: nothing is allocated or synchronised and no
 * library workspace is taken; the caller's workspace is the only scratch.
 * The record is deterministic whichever wave sees an offence.  Nothing outside
 * [d_in, d_in + nchars) is read, the wide loads at the head and tail of an
 * unaligned text included; nothing outside the output capacity, the record
 * and the workspace is written.  Any alignment of the text and the output is
 * accepted; no 32-bit limit on nchars.  The finish step walks back from the
 * end of the text to its last three kept bytes 1,024 bytes at a time in one
 * wave: a text that ends in a very long run of skipped bytes is exact but is
 * walked at that one wave's rate. */
int b64x_decode_strict_skip_dev(const void *d_in, uint64_t nchars,
                                void *d_out /* NULL: validate only */, b64x_strict_result *d_res,
                                const b64x_alphabet *abc, const b64x_skip *skip,
                                void *d_workspace, void *stream);

/* Ragged batch, addressed as b64x_decode_strict_batch: text i is judged on
 * its own, err_pos an offset inside the buffer, its bytes (d_out not NULL)
 * at d_out + d_out_off[i] with capacity b64x_decoded_cap(len_i).  Lengths are
 * read on the device: the checking kernel's grid and arguments depend on
 * nbuf, abc and skip only.  One wave judges one buffer, in passes of 1,024
 * bytes, and writes its record whole; a buffer of hundreds of MiB is exact but
 * runs at one wave's rate and belongs on the one-buffer call.  With d_out not
 * NULL the bytes come from b64x_decode_batch on the same offsets, its
 * d_outlen being d_workspace (8 nbuf bytes, 8-byte aligned); the record's
 * out_len is the checking kernel's own, 0 on an offence.
 * Checked in this order: nbuf == 0 returns 0; NULL d_in, d_in_off or d_res
 * (or records not 8-byte aligned) -EINVAL, and with d_out not NULL a NULL
 * d_out_off or d_workspace too (a validate-only batch needs neither); the
 * skip set; the alphabet; then -ENODEV. */
int b64x_decode_strict_skip_batch(const void *d_in, const uint64_t *d_in_off, uint32_t nbuf,
                                  void *d_out /* NULL: validate only */,
                                  const uint64_t *d_out_off,
                                  b64x_strict_result *d_res /* nbuf */,
                                  const b64x_alphabet *abc, const b64x_skip *skip,
                                  void *d_workspace /* 8*nbuf bytes; unused when d_out is NULL */,
                                  void *stream);

/* Uniform rows, addressed as b64x_decode_strict_strided: row i is the `len`
 * bytes at d_in + i*in_stride, judged on its own by the scalar procedure above
 * (steps 1 to 6); its record goes to d_res[i], err_pos an offset in the row.
 * `abc` is read as the strict decoder reads it, skip NULL means CR and LF,
 * B64X_STRICT_SEP is never reported.  With d_out not NULL an accepted row's
 * out_len bytes go to d_out + i*out_stride (capacity b64x_decoded_cap(len));
 * with an offence out_len is 0 and the row's output bytes are unspecified.
 * len == 0 is valid: every record is {0, 0, OK}.  Added within ABI 7 (a
 * symbol only).
 * One pass, one kernel: the wave that owns a row reads its text once, in
 * passes of 1,024 bytes, compacts the kept characters and decodes them
 * itself, and writes the record whole (the caller need not zero the records).
 * Unlike the two calls above there is no workspace and the lenient decoder
 * takes no part.  For row i nothing is written outside [d_out + i*out_stride,
 * + b64x_decoded_cap(len)) and the records, and nothing is read outside the
 * row's len bytes, the wide loads at an unaligned row's head and tail
 * included.  Input and output must not overlap.  Any alignment of the base
 * addresses and of the strides is accepted; rows whose input and output
 * addresses are both 4-byte aligned are the fast shape.  No 32-bit limit on
 * len, the strides or i*stride -- but one wave walks one row, so a row of
 * hundreds of MiB, exact as it is, runs at one wave's rate (the kernel
 * balances a batch over rows, not over the bytes of one): such a text belongs
 * on b64x_decode_strict_skip_dev.
 * Asynchronous, capture-safe and exact: no workspace, no allocation, no
 * synchronisation, no library state, no hint; no memset node and no global
 * atomic.
 * Checked in this order: nbuf == 0 returns 0; a NULL d_in or d_res (or records
 * not 8-byte aligned) -EINVAL; in_stride < len -EINVAL; with d_out not NULL,
 * out_stride < b64x_decoded_cap(len) -EINVAL; the skip-set rules of
 * b64x_decode_strict_skip_dev; the alphabet rules of b64x_decode_strict_dev;
 * then -ENODEV without a gfx950 device. */
int b64x_decode_strict_skip_strided(const void *d_in, uint64_t in_stride, uint64_t len, uint32_t nbuf,
                                    void *d_out /* NULL: validate only */, uint64_t out_stride,
                                    b64x_strict_result *d_res /* nbuf */,
                                    const b64x_alphabet *abc, const b64x_skip *skip, void *stream);

/* Texts that arrive in pieces: the strict skip decode, continued from block
 * to block.  Many streams go in one launch; each has a state in device memory
 * and contributes one piece, read once by the wave that owns it.  Added
 * within ABI 7 (symbols only).
 *
 * State.  Its contents are the library's own.  128 bytes of zero mean "start
 * of a text", so a caller arms states with a memset.  Piece i continues the
 * text of state d_state[d_sid ? d_sid[i] : i]; the state indices of one call
 * must be distinct (not checked), and the order between calls is stream
 * order.  A piece with d_flags[i] & B64X_PIECE_FINAL ends its text and leaves
 * the state all zero again, ready for the next text.
 *
 * The result is what the scalar procedure of b64x_decode_strict_skip_dev
 * gives for the concatenation T of the pieces one state has taken so far:
 *  1. Every piece adds its kept bytes to the state's totals (E, the count c
 *     of pad characters, the lowest offset of a stranger and of a pad
 *     character, the last three kept bytes with their offsets; offsets are
 *     offsets in T).  With npad the pad characters T ends in so far (0..2; 0
 *     without pad): if c > npad and the first pad character lies below the
 *     first stranger the record is {0, first_pad, PAD}; otherwise, with a
 *     stranger, {0, first_char, CHAR}.  Such an early report is final -- PAD
 *     and CHAR can only become more true as T grows -- and the state keeps
 *     it: every later piece of that text gets the same record, writes no
 *     output and need not be read (no more than its first pass of 1,024 bytes
 *     is loaded, and nothing of it is looked at).
 *  2. A piece that is not final, without an offence: k = the sextets carried
 *     (0..3) plus the piece's data characters; it writes the 3 floor(k/4)
 *     bytes of the whole groups, keeps k mod 4 sextets in the state, and its
 *     record is {3 floor(k/4), 0, OK}.
 *  3. A final piece without an offence so far judges LENGTH (err_pos = |T|),
 *     then BITS (at the offset in T of kept byte D-1, which may lie in an
 *     earlier piece); if accepted it writes the whole groups and the 1 or 2
 *     bytes of the last partial group.  out_len is the bytes this piece
 *     wrote: over all pieces the written bytes, concatenated, are exactly the
 *     bytes b64x_decode_strict_skip_dev gives for T, and the out_len values
 *     sum to its out_len.
 *  4. An empty piece is valid: one that is not final changes nothing, a final
 *     one finishes the text.  A piece of skipped bytes only likewise.
 *
 * Piece i is d_in[d_in_off[i] .. d_in_off[i+1]) and writes at d_out +
 * d_out_off[i], capacity b64x_skip_piece_cap(len_i) = b64x_decoded_cap(len_i
 * + 3): a final piece of 4 characters behind a carry of 3 writes 5 bytes.
 * Nothing is written outside the capacities, the records and the states
 * named; nothing is read outside the pieces and the states named, the wide
 * loads at an unaligned piece's edges included.  With an offence the output
 * bytes inside the capacity are unspecified.  Input and output must not
 * overlap; any alignment is accepted; offsets and |T| are 64-bit.
 * Checked in this order: npieces == 0 returns 0; a NULL d_in, d_in_off,
 * d_state or d_res, or records or states not 8-byte aligned, -EINVAL; with
 * d_out not NULL a NULL d_out_off -EINVAL; the skip-set rules of
 * b64x_decode_strict_skip_dev; the alphabet rules of b64x_decode_strict_dev;
 * then -ENODEV without a gfx950 device.
 * Asynchronous and capture-safe: lengths, flags and state indices are read on
 * the device, grid and kernel arguments depend on npieces, abc and skip only,
 * so a captured call replays on other lengths, flags and indices.  No
 * workspace, no allocation, no library state, no memset node, no atomic.
 * Known limit: one wave walks one piece, so a piece of many MiB is exact but
 * runs at one wave's rate, as with every batch call here: such a piece belongs
 * on b64x_decode_strict_skip_piece_dev below, which continues the same state.
 * The encode side needs no such call: a caller who cuts the input at
 * multiples of 3 L/4 bytes and sets B64X_LINES_TRAILING gets a continuable
 * b64x_encode_lines_*. */
#define B64X_SKIP_STATE_BYTES 128
typedef struct b64x_skip_state {
    uint64_t w[16];
} b64x_skip_state; /* device memory, 8-byte aligned */
#define B64X_PIECE_FINAL 1u

/* Output capacity of a piece of len bytes: b64x_decoded_cap(len + 3). */
uint64_t b64x_skip_piece_cap(uint64_t len);

int b64x_decode_strict_skip_pieces(const void *d_in, const uint64_t *d_in_off, uint32_t npieces,
                                   void *d_out /* NULL: validate only */,
                                   const uint64_t *d_out_off /* npieces */,
                                   b64x_skip_state *d_state,
                                   const uint32_t *d_sid /* NULL: piece i continues state i */,
                                   const uint8_t *d_flags /* NULL: no piece is final */,
                                   b64x_strict_result *d_res /* npieces */,
                                   const b64x_alphabet *abc, const b64x_skip *skip, void *stream);

/* One large piece of one text, spread over the GPU.  The call does what
 * b64x_decode_strict_skip_pieces does for npieces == 1 with the piece
 * d_in[0 .. len), the state d_state[0], d_out_off[0] == 0 and d_flags[0] ==
 * flags: the same record, and the same bytes at d_out with capacity
 * b64x_skip_piece_cap(len).  A final piece on a zeroed state is
 * b64x_decode_strict_skip_dev without the lenient decoder.  Added within ABI 7
 * (symbols only).
 * A state that holds a report repeats it: nothing of the piece is looked at
 * and nothing is written except the record, the first 8 bytes of the
 * workspace and, for a final piece, the zeroed state.  The two calls may be
 * interleaved on one state in any order: after a piece that is not final and
 * has no offence, state words 0 to 10 are byte for byte what the pieces call
 * leaves in the same mode (decoding or validate only; the pieces call keeps
 * the carried sextets in a decoding call only, so a text stays in one mode),
 * words 11 to 15 stay zero; after a piece that reports PAD or CHAR words 9 and
 * 10 hold the report, which is all either call reads of such a state; after a
 * final piece all 16 words are zero.
 * Three launches in stream order -- a count pass with a wave per tile of the
 * piece, a scan of the tiles' records with the verdict and the new state in
 * one workgroup, a decode pass with a wave per tile (not with d_out NULL) --
 * and no hand-off between workgroups inside one.  The text is read twice by a
 * decoding call and once by a validate-only one.
 * len is a host value and the grid depends on it, so a captured call replays
 * on the same length (and the same address modulo 16) only, with any
 * contents, state and flags' outcome; b64x_decode_strict_skip_batch and the
 * pieces call remain the ones that replay on other lengths.
 * d_workspace: b64x_strict_skip_piece_workspace_size(len, d_out == NULL)
 * bytes of device memory, 8-byte aligned, one per stream.  It needs no
 * preparation: every word the call reads it wrote earlier in the same call.
 * The size is a head of 64 bytes and 64 bytes per tile, at most 1 MiB + 64;
 * today it is the same for both modes.
 * Asynchronous and capture-safe: no allocation, no synchronisation, no
 * library state, no memset node, no global atomic.  Any alignment of the text
 * and the output is accepted; no 32-bit limit on len.  Nothing outside [d_in,
 * d_in + len) and the state is read, the wide loads at unaligned edges
 * included; nothing outside the output capacity, the record, the state and
 * the workspace is written.  With an offence the decode pass does not run and
 * the output is untouched.  Input and output must not overlap.  The scan
 * walks back from the end of the piece to its last three kept bytes 1,024
 * bytes at a time in one wave, as b64x_decode_strict_skip_dev does: a piece
 * that ends in a very long run of skipped bytes is exact but is walked at
 * that one wave's rate.
 * Checked in this order: a NULL d_in, d_state, d_res or d_workspace, or a
 * record, state or workspace not 8-byte aligned, -EINVAL -- d_out may be NULL,
 * and len == 0 still wants a d_in; flags with a bit other than
 * B64X_PIECE_FINAL -EINVAL; the skip-set rules of
 * b64x_decode_strict_skip_dev; the alphabet rules of b64x_decode_strict_dev;
 * then -ENODEV without a gfx950 device. */
uint64_t b64x_strict_skip_piece_workspace_size(uint64_t len, bool validate_only);

int b64x_decode_strict_skip_piece_dev(const void *d_in, uint64_t len,
                                      void *d_out /* NULL: validate only */,
                                      b64x_skip_state *d_state, unsigned flags /* B64X_PIECE_FINAL */,
                                      b64x_strict_result *d_res,
                                      const b64x_alphabet *abc, const b64x_skip *skip,
                                      void *d_workspace, void *stream);

/* Many pieces of any size in one call: b64x_decode_strict_skip_pieces with a
 * wave on every tile of every piece, as b64x_decode_strict_skip_piece_dev puts
 * one on every tile of its piece, in a constant number of launches.  Added
 * within ABI 7 (symbols only).
 * For every piece the record, the bytes written at d_out + d_out_off[i]
 * (capacity b64x_skip_piece_cap(len_i)) and the state left behind are those of
 * b64x_decode_strict_skip_pieces with the same arguments: state words 0 to 10
 * byte for byte the same in the same mode, words 11 to 15 zero, all 16 zero
 * after a final piece; after a piece that reports PAD or CHAR words 9 and 10
 * hold the report, which is all any of the calls reads of such a state.  The
 * three calls may take turns on one state in any order.  A state that holds a
 * report repeats it and nothing of that piece is looked at: no more than the
 * first pass of 1,024 bytes of each of its tiles is loaded, as the pieces call
 * loads a piece's first pass before it knows the state.  Stronger than the pieces call: a piece whose record carries an
 * offence, held or new, writes nothing to its output -- the decode pass runs
 * behind the verdict.
 * total_cap is a host bound on d_in_off[npieces] - d_in_off[0]; the size of
 * the caller's text buffer will do.  It is the only length the host sees: tile
 * size, grids, kernel arguments and workspace size are functions of total_cap,
 * npieces, abc, skip and d_out == NULL alone, so a captured call replays on
 * other lengths, flags, state indices and contents within the same bound.  If
 * the device finds d_in_off[npieces] - d_in_off[0] > total_cap, no piece is
 * looked at, no state and no output byte is touched, and every record is
 * {0, d_in_off[npieces] - d_in_off[0], B64X_STRICT_BOUND}.
 * Four launches in stream order (three with d_out NULL): a prefix over the
 * pieces' tile counts in one workgroup, which also maps every tile to its
 * piece; a count pass with a wave per tile; a scan per piece -- a wave for a
 * piece of up to 64 tiles, a workgroup for a longer one -- with the verdict
 * and the new state; a decode pass with a wave per tile.  The text is read
 * twice by a decoding call and once by a validate-only one, so a batch of
 * single-tile pieces is cheaper on b64x_decode_strict_skip_pieces.
 * d_workspace: b64x_strict_skip_pieces_wide_workspace_size(total_cap, npieces,
 * d_out == NULL) bytes of device memory, 8-byte aligned, one per stream, no
 * preparation: 64 bytes per piece, 72 bytes per tile of the bound
 * ceil(total_cap / T) + 2 npieces, and small change.
 * Any alignment of text and output; 64-bit offsets and |T|; input and output
 * must not overlap; the state indices of one call are distinct (not checked).
 * Nothing outside the pieces, states and workspace is read, the wide loads at
 * unaligned edges included; nothing outside capacities, records, states and
 * workspace is written.  Asynchronous and capture-safe: no allocation, no
 * synchronisation, no library state, no memset node, no global atomic, no spin
 * or hand-off between workgroups inside a launch.
 * Checked in this order: npieces == 0 returns 0; a NULL d_in, d_in_off,
 * d_state, d_res or d_workspace, or records, states or workspace not 8-byte
 * aligned, -EINVAL; with d_out not NULL a NULL d_out_off -EINVAL; the skip-set
 * rules of b64x_decode_strict_skip_dev; the alphabet rules of
 * b64x_decode_strict_dev; then -ENODEV without a gfx950 device. */
#define B64X_STRICT_BOUND 6u  /* the call's pieces are longer than the bound the caller gave; nothing was looked at */

uint64_t b64x_strict_skip_pieces_wide_workspace_size(uint64_t total_cap, uint32_t npieces, bool validate_only);

int b64x_decode_strict_skip_pieces_wide(const void *d_in, const uint64_t *d_in_off, uint32_t npieces,
                                        uint64_t total_cap,
                                        void *d_out /* NULL: validate only */,
                                        const uint64_t *d_out_off /* npieces */,
                                        b64x_skip_state *d_state,
                                        const uint32_t *d_sid /* NULL: piece i continues state i */,
                                        const uint8_t *d_flags /* NULL: no piece is final */,
                                        b64x_strict_result *d_res /* npieces */,
                                        const b64x_alphabet *abc, const b64x_skip *skip,
                                        void *d_workspace, void *stream);

/* ---- host-memory sessions (used by the bytestream_1 stages) ----------- */

typedef struct b64x_session b64x_session;

/* A session owns a HIP stream, pinned host staging of `capacity` input
 * bytes/characters and matching device buffers.  NULL + errno on
 * failure (ENODEV when no GPU is usable). */
b64x_session *b64x_session_open(uint64_t capacity);
void b64x_session_close(b64x_session *s);
uint64_t b64x_session_capacity(const b64x_session *s);
/* Pooled form: acquire takes an idle session of this capacity on the
 * current device from a process-wide pool (opening one if there is none);
 * release waits for the session's queued work and returns it to the pool
 * (closing it when the pool is full).  Opening a session costs pinned
 * allocations and a HIP stream -- milliseconds -- so stages that come and
 * go per message reuse them. */
b64x_session *b64x_session_acquire(uint64_t capacity);
void b64x_session_release(b64x_session *s);
/* Pinned host staging areas: fill host_in, read results from host_out. */
uint8_t *b64x_session_host_in(b64x_session *s);
uint8_t *b64x_session_host_out(b64x_session *s);

/* Synchronous round trips host_in[0..n) -> GPU -> host_out.  The encoder
 * leg encodes all n bytes (padding the final group iff `final` and
 * abc->pad); the caller passes whole 3-byte groups unless `final`.  The
 * decoder leg honours `flags` as b64x_decode_dev(). */
int b64x_session_encode(b64x_session *s, uint64_t n,
                        const b64x_alphabet *abc, uint64_t *out_len);
int b64x_session_decode(b64x_session *s, uint64_t n,
                        const b64x_alphabet *abc, unsigned flags,
                        b64x_dec_result *res);

/* Completion callback of the asynchronous session calls.  It runs on a HIP
 * runtime thread and must not call HIP; it should only signal (set a flag,
 * write an eventfd). */
typedef void (*b64x_done_fn)(void *arg);

/* Asynchronous forms of b64x_session_encode/_decode: enqueue H2D, kernels
 * and D2H on the session's stream and return at once.  `done(arg)` (may be
 * NULL) runs once the call's work has finished; for decode, read the
 * result with b64x_session_decode_result().  One call in flight per
 * session. */
int b64x_session_encode_async(b64x_session *s, uint64_t n,
                              const b64x_alphabet *abc, b64x_done_fn done,
                              void *arg);
/* A caller that decodes one stream in several blocks uses
 * B64X_DEC_HOLD_TAIL and spells the record's held-back sextets in front of
 * its next block itself (ABI version 1's device-side chaining of sessions,
 * `carry_from`, is gone: DESIGN.md §8, "Round 1's decoder-ingress block
 * loss"). */
int b64x_session_decode_async(b64x_session *s, uint64_t n,
                              const b64x_alphabet *abc, unsigned flags,
                              b64x_done_fn done, void *arg);
/* The decode result of the last completed call (host memory; the kernels
 * write it there themselves).  Raw view: prefer the checked form below. */
const b64x_dec_result *b64x_session_result(const b64x_session *s);
/* Checked copy of the last decode's result, to be called once its `done`
 * has run (or after b64x_session_wait).  The record is poisoned before each
 * launch; one that is still poisoned, names another call (seq, nchars or
 * flags differ) or is inconsistent (valid > characters, tail_n != valid
 * mod 4, a held-back sextet >= 64 or a nonzero unused tail byte, out_len
 * not the flags' function of valid) is counted (b64x_diag_counters), the
 * session's stream is waited for and the record is checked again.  0, or
 * -EIO if it is still wrong. */
int b64x_session_decode_result(b64x_session *s, b64x_dec_result *res);
/* Wait for everything queued on the session. */
int b64x_session_wait(b64x_session *s);

/* ---- batch lanes (cross-stream batching of host blocks) --------------- */

/* Pinned host memory for batch arenas (hipHostMalloc, fine-grained); NULL
 * on failure. */
void *b64x_host_alloc(uint64_t bytes);
void b64x_host_free(void *p);

/* A lane: one HIP stream plus device buffers that grow on demand.  It
 * runs ragged batches out of caller-owned pinned arenas; the bytestream_1
 * stages pack many streams' blocks into one batch so that a launch (and
 * its one H2D copy) is amortised over them (ref
 * src/queuestream.c:150-191 being the per-message feed).  The kernels
 * write every output -- characters, bytes, result records -- straight into
 * the pinned host buffers: there is no D2H copy to trust.  After a batch's
 * `done(arg)` has run, the caller checks it with b64x_lane_encode_check /
 * b64x_lane_decode_check before reading anything. */
typedef struct b64x_lane b64x_lane;

b64x_lane *b64x_lane_open(void);
void b64x_lane_close(b64x_lane *l);
/* Pooled form (see b64x_session_acquire): an idle lane of the current
 * device from the process-wide pool, or a new one; release waits for the
 * lane's queued work and pools it. */
b64x_lane *b64x_lane_acquire(void);
void b64x_lane_release(b64x_lane *l);
/* Encode njobs buffers: buffer i is h_in[h_in_off[i] .. h_in_off[i+1])
 * and its b64x_encoded_len(len, abc->pad) characters go to
 * h_out + h_out_off[i] (both offset arrays hold njobs+1 monotone entries
 * starting at 0).  All four host buffers must be pinned (b64x_host_alloc)
 * and stay untouched until `done(arg)` has run.  Asynchronous; the lane's
 * device buffers are grown (synchronously) when a batch needs more.  One
 * batch in flight per lane.
 *
 * h_seg[0 .. nseg) (pinned; nseg may be 0): parts of the batch's input
 * that are not in h_in but elsewhere in pinned host memory -- the input's
 * bytes [off, off+len) are at src (h_in's bytes there are not read) --
 * sorted by off, not overlapping.  A batch with segments is gathered into
 * the device by one kernel that reads h_in and the segments straight from
 * host memory (no DMA of h_in). */
typedef struct {
    uint64_t off, len;
    const uint8_t *src;
} b64x_seg;
int b64x_lane_encode_async(b64x_lane *l, const uint8_t *h_in, uint32_t njobs,
                           const uint64_t *h_in_off, uint8_t *h_out,
                           const uint64_t *h_out_off, const b64x_seg *h_seg, uint32_t nseg,
                           const b64x_alphabet *abc, b64x_done_fn done, void *arg);
/* The encode batch whose `done` has run really finished: its completion
 * stamp (written by a kernel queued behind the encode) is there; if not,
 * counted (b64x_diag_counters), waited for and checked again.  0 or -EIO. */
int b64x_lane_encode_check(b64x_lane *l);
/* Lane decode job flag (h_flags): the job is chained -- h_prev[i] names the
 * record whose held-back sextets complete its 4-byte head (below). */
#define B64X_LANE_CHAINED 4u

/* Decode njobs character buffers: job i is h_in[h_in_off[i] ..
 * h_in_off[i+1]), its bytes go to h_out + h_out_off[i] (capacity
 * >= b64x_decoded_cap(len)) and its result record to h_res[i].  h_flags[i]
 * & B64X_DEC_HOLD_TAIL: more of the job's stream follows, so only whole
 * groups are emitted and the last V mod 4 sextets are reported in the
 * record (b64x_decode_dev's HOLD_TAIL); otherwise the job ends its stream
 * and its final partial group is emitted.  Pinned host buffers, as for
 * b64x_lane_encode_async; the records are poisoned here.  *seq receives
 * the batch's sequence number (its records' `seq`; pass it to
 * b64x_lane_decode_check).
 *
 * Chained jobs (one stream decoded in blocks without waiting for each
 * block's record on the host): h_flags[i] & B64X_LANE_CHAINED and h_prev[i]
 * (h_prev may be NULL when no job is chained) points at the pinned host
 * record of an earlier HOLD_TAIL job of the same stream -- in this batch or
 * in a batch queued before it on this lane.  Job i's first 4 characters are
 * a head of characters outside the alphabet; on the device, after that
 * record has been written and before job i is decoded, its last tail_n
 * head bytes are replaced by the record's held-back sextets spelled as
 * alphabet characters, and what was spelled from is logged to h_spell[i]
 * (pinned), which b64x_lane_decode_check compares with the record.
 * Chained jobs and jobs of 128 KiB or more are decoded one after another
 * in job order; the rest in one batch launch before them.
 *
 * Several decode batches may be queued on one lane; they run in order.
 * Encode batches only go to an idle lane. */
int b64x_lane_decode_async(b64x_lane *l, const uint8_t *h_in, uint32_t njobs,
                           const uint64_t *h_in_off, uint8_t *h_out,
                           const uint64_t *h_out_off, const uint8_t *h_flags,
                           b64x_dec_result *h_res, const b64x_dec_result *const *h_prev,
                           b64x_dec_result *h_spell, const b64x_alphabet *abc,
                           b64x_done_fn done, void *arg, uint32_t *seq);
/* Checks a finished decode batch's records (see b64x_session_decode_result
 * for what is checked) and, for chained jobs, that the head was spelled
 * from the finished predecessor record: one still poisoned or inconsistent
 * is counted, the lane is waited for and the records are checked again.  0
 * or -EIO. */
int b64x_lane_decode_check(b64x_lane *l, uint32_t seq, const uint64_t *h_in_off,
                           const uint8_t *h_flags, const b64x_dec_result *h_res,
                           const b64x_dec_result *const *h_prev,
                           const b64x_dec_result *h_spell, uint32_t njobs);
/* Wait for everything queued on the lane. */
int b64x_lane_wait(b64x_lane *l);

/* Completion results found unfinished when their `done` had already run:
 * out[0] session decode records, out[1] lane batches (process-wide totals,
 * for tests and diagnostics). */
void b64x_diag_counters(uint64_t out[2]);
/* Paths the automatic decodes took (process-wide totals, for tests and
 * diagnostics): out[0] probes launched, out[1] probes skipped on a held
 * model, out[2] hinted single passes, out[3] row-batch preps launched,
 * out[4] row-batch preps skipped (the workspace's row model reused). */
void b64x_diag_paths(uint64_t out[5]);

/* ---- utilities ----------------------------------------------------------- */

/* Fill n bytes with the splitmix64 stream used by every synthetic
 * workload: 8 little-endian bytes per step,
 * state = seed + k*0x9E3779B97F4A7C15 for k = 1, 2, ... */
int b64x_fill_splitmix64(void *d_out, uint64_t n, uint64_t seed,
                         void *stream);

/* 0 if a gfx950 device is usable, -ENODEV otherwise. */
int b64x_device_check(void);

/* ---- host placement ------------------------------------------------------ */

/* The NUMA node the GPU `device` (-1: the current device) hangs off, from
 * sysfs; -ENOENT when unknown (no NUMA, a virtual device).  */
int b64x_device_numa_node(int device);
/* Bind the calling thread to the CPUs of `device`'s NUMA node (-1: the
 * current device) that its affinity mask allows, and prefer that node for
 * the pages it faults in.  Event loops that feed a GPU spend their time
 * copying messages into pinned arenas and reading frames back: one loop ran
 * config 5 at 6.1-6.2 GiB/s on the GPU's node and 4.4-4.5 on the other
 * socket of the same box (profiles/r06_numa_probe.jsonl).  A thread whose
 * mask already lies inside one node (the application placed it) is left as
 * it is.  Returns the node the thread runs on afterwards, or a negative errno
 * (-ENOENT: the node or its CPUs are unknown; the thread is unchanged).  The
 * batching hub calls it on a loop's thread when the loop gets its first GPU
 * stage, unless ASYNC_B64_BIND=0. */
int b64x_bind_thread(int device);
/* Static description of the compiled kernels (for logs). */
const char *b64x_build_info(void);
const char *b64x_strerror(int err);

#ifdef __cplusplus
}
#endif

#endif /* ASYNC_AMD_B64X_H */
