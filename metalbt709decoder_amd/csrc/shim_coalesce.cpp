// C-ABI shim, the coalescing submit (include/bt709hip_ext.h, BT709HIP_OPT_COALESCE): a decoder that keeps the reference's
// one -decodeBT709: call per frame validates each call at once but gathers the frames of a stream into one launch.
#include "shim_internal.h"

namespace bt709shim __attribute__((visibility("hidden"))) {

// Launches what `q` holds (dec->queue_mutex held).  The queue is emptied first: a failed launch is reported once, to the
// call that issued it, and never re-issued.
int issue_queue(bt709hip_decoder *dec, PendingQueue &q) {
  if (q.frames.empty()) return BT709HIP_OK;
  std::vector<bt709hip_frame> frames, alphas;
  std::vector<bt709hip_surface> outs;
  frames.swap(q.frames);
  alphas.swap(q.alphas);
  outs.swap(q.outs);
  return decode_batch_now(dec, q.layout, static_cast<int>(frames.size()), frames.data(), q.with_alphas ? alphas.data() : nullptr, outs.data(),
                          q.stream, 0);
}

namespace {
int64_t now_us() {
  return std::chrono::duration_cast<std::chrono::microseconds>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
}  // namespace

// one decoder: the queue of stream `s`, or every queue (all = true); aged_only: only queues older than the decoder's age limit
int flush_decoder(bt709hip_decoder *dec, hipStream_t s, bool all, bool aged_only) {
  std::lock_guard<std::mutex> lock(dec->queue_mutex);
  int rc = BT709HIP_OK;
  const int64_t limit = aged_only ? now_us() - dec->coalesce_max_age_us : 0;
  for (PendingQueue &q : dec->queues) {
    if (q.frames.empty()) continue;
    const bool aged = dec->coalesce_max_age_us > 0 && q.oldest_us <= limit;
    if (aged_only ? (aged || q.stream == s) : (all || q.stream == s))
      if (int e = issue_queue(dec, q)) rc = rc ? rc : e;
  }
  return rc;
}

// Every coalescing decoder of `ctx` except `skip`: called by each entry point that takes a stream, before it touches the stream
// -- the queue of THAT stream goes out (stream order), and so does any queue of any stream that has outlived its decoder's
// BT709HIP_OPT_COALESCE_MAX_AGE_US (nothing here runs on a timer: an idle caller's frames wait for the context's next call).
// coalescing_mutex is held across the loop (lock order: coalescing_mutex, then a decoder's queue_mutex): a decoder that is being
// destroyed leaves the list under the same mutex (set_coalescing), so none of the pointers can dangle.
int flush_stream(bt709hip_context *ctx, hipStream_t s, const bt709hip_decoder *skip) {
  if (ctx == nullptr || ctx->n_coalescing.load(std::memory_order_acquire) == 0) return BT709HIP_OK;
  // While the CALLING stream records a graph only its own queue goes out: an aged queue of another stream may need a first-use
  // table (an allocation + blocking copies: illegal on a thread that is capturing) and has nothing to do with this recording;
  // it waits for the context's next call outside a capture.
  const bool aged_too = !capturing(s);
  // SERIALISATION: coalescing_mutex is held across the launches the loop issues, so while at least one decoder of the context
  // coalesces, the context's stream-taking entry points run one at a time for the length of those (asynchronous, ~10 us) launch
  // calls.  Contexts without a coalescing decoder never take the mutex (the counter above).
  std::lock_guard<std::mutex> lock(ctx->coalescing_mutex);
  int rc = BT709HIP_OK;
  for (bt709hip_decoder *d : ctx->coalescing)
    if (d != skip)
      if (int e = flush_decoder(d, s, false, aged_too)) rc = rc ? rc : e;
  return rc;
}

// Turns the coalescing submit of `dec` on (n > 1), off (0) or changes its count.  Order matters when other threads are inside a
// decode: ON registers the decoder with its context BEFORE the count becomes visible (a frame queued from then on is seen by
// every flush_stream), OFF issues what is queued and clears the count under the queue_mutex -- a submit that is waiting for that
// mutex re-reads the count behind it and launches instead of queueing -- and only then leaves the context's list.  Lock order:
// the context's coalescing_mutex and a decoder's queue_mutex are never held together here.  Returns the flush's status.
int set_coalescing(bt709hip_decoder *dec, int n) {
  bt709hip_context *ctx = dec->ctx;
  const bool now = n > 1;
  if (now && ctx != nullptr) {
    std::lock_guard<std::mutex> lock(ctx->coalescing_mutex);
    if (std::find(ctx->coalescing.begin(), ctx->coalescing.end(), dec) == ctx->coalescing.end()) ctx->coalescing.push_back(dec);
    ctx->n_coalescing.store(static_cast<int>(ctx->coalescing.size()), std::memory_order_release);
  }
  int rc = BT709HIP_OK;
  {
    std::lock_guard<std::mutex> lock(dec->queue_mutex);
    if (!now)  // off: nothing may stay queued behind the switch
      for (PendingQueue &q : dec->queues)
        if (int e = issue_queue(dec, q)) rc = rc ? rc : e;
    dec->coalesce.store(now ? n : 0);
  }
  if (!now && ctx != nullptr) {
    std::lock_guard<std::mutex> lock(ctx->coalescing_mutex);
    auto it = std::find(ctx->coalescing.begin(), ctx->coalescing.end(), dec);
    if (it != ctx->coalescing.end()) ctx->coalescing.erase(it);
    ctx->n_coalescing.store(static_cast<int>(ctx->coalescing.size()), std::memory_order_release);
  }
  return rc;
}

namespace {
bool same_shape(const bt709hip_frame &a, const bt709hip_frame &b) {
  return a.width == b.width && a.height == b.height && a.y_stride == b.y_stride && a.cbcr_stride == b.cbcr_stride;
}

// STREAM ORDER BETWEEN CALLS.  The items of one launch run concurrently, so a call may only join a queue when it neither
// writes a byte a queued call reads or writes nor reads a byte a queued call writes; otherwise the queue goes out first, as
// for a change of geometry.  (Overlap INSIDE one batch call stays the caller's error, as without the option.)
bool meet(const ByteSpan &a, const ByteSpan &b) { return a.lo < b.hi && b.lo < a.hi; }

void join(ByteSpan &a, const ByteSpan &b) {
  a.lo = std::min(a.lo, b.lo);
  a.hi = std::max(a.hi, b.hi);
}

ByteSpan plane_span(const void *base, size_t rows, size_t stride, size_t row_bytes) {
  const uintptr_t b = reinterpret_cast<uintptr_t>(base);
  return ByteSpan{b, b + (rows - 1) * stride + row_bytes};
}

// what a (non-empty) item reads: Y, the chroma -- CbCr rows, or the U plane and the V plane (H/2) * cbcr_stride behind it as
// one range -- and the alpha plane where the decoder reads one
struct ItemReads {
  ByteSpan plane[3];
};
ItemReads reads_of(const bt709hip_frame &f, const bt709hip_frame *a, int layout) {
  const size_t w = static_cast<size_t>(f.width), h = static_cast<size_t>(f.height);
  ItemReads r;
  r.plane[0] = plane_span(f.y, h, f.y_stride, w);
  r.plane[1] = layout == BT709HIP_CHROMA_I420 ? plane_span(f.cbcr, h, f.cbcr_stride, w / 2) : plane_span(f.cbcr, h / 2, f.cbcr_stride, w);
  if (a != nullptr) r.plane[2] = plane_span(a->y, h, a->y_stride, w);
  return r;
}

size_t row_bytes_of(const bt709hip_surface &o) { return static_cast<size_t>(o.width) * (o.format == BT709HIP_FORMAT_RGBA16F ? 8 : 4); }

ByteSpan write_of(const bt709hip_surface &o) { return plane_span(o.bgra, static_cast<size_t>(o.height), o.stride, row_bytes_of(o)); }

// Two targets of one pitch, height and row length.  Where the later one's rows lie on the earlier one's pitch grid (windows of
// one canvas) the rectangles are compared, exactly; where they straddle the grid's rows, the byte ranges.
bool targets_meet(const bt709hip_surface &p, const bt709hip_surface &q) {
  uintptr_t a = reinterpret_cast<uintptr_t>(p.bgra), b = reinterpret_cast<uintptr_t>(q.bgra);
  if (a > b) std::swap(a, b);
  const size_t rows = static_cast<size_t>(p.height), row = row_bytes_of(p);
  const uintptr_t d = b - a;
  const size_t dy = d / p.stride, dx = d % p.stride;
  if (dx + row <= p.stride) return dy < rows && dx < row;
  return d < (rows - 1) * p.stride + row;
}

// `alphas`: the alpha frames the decoder READS (nullptr for an opaque decoder, whatever the caller passed).  The call fits the
// queue: one geometry, pitches, format and layout on both sides, alpha frames passed on both or on neither.
bool conflicts(const PendingQueue &q, const ByteSpan &writes, const ByteSpan &reads, int count, const bt709hip_frame *frames,
               const bt709hip_frame *alphas, const bt709hip_surface *outs) {
  if (!meet(writes, q.writes) && !meet(writes, q.reads) && !meet(reads, q.writes)) return false;  // the usual case: slots of a ring
  for (size_t j = 0; j < q.frames.size(); ++j) {
    const ItemReads qr = reads_of(q.frames[j], alphas ? &q.alphas[j] : nullptr, q.layout);
    const ByteSpan qw = write_of(q.outs[j]);
    for (int i = 0; i < count; ++i) {
      if (targets_meet(q.outs[j], outs[i])) return true;
      const ItemReads r = reads_of(frames[i], alphas ? &alphas[i] : nullptr, q.layout);
      const ByteSpan w = write_of(outs[i]);
      for (int k = 0; k < 3; ++k)
        if (meet(r.plane[k], qw) || meet(w, qr.plane[k])) return true;
    }
  }
  return false;
}
}  // namespace

// BT709HIP_OPT_COALESCE (include/bt709hip_ext.h, COALESCING SUBMIT): validate now, launch later.
int coalescing_submit(bt709hip_decoder *dec, int layout, int count, const bt709hip_frame *frames, const bt709hip_frame *alphas,
                      const bt709hip_surface *outs, void *stream, int wait_until_completed) {
  if (dec->ctx == nullptr) return decode_batch_now(dec, layout, count, frames, alphas, outs, stream, wait_until_completed);
  hipStream_t s = pick(dec->ctx, stream);
  // what the context's OTHER coalescing decoders have queued for this stream was submitted before this call: it goes first.
  // Done before this decoder's own queue_mutex is taken (lock order: the context's coalescing_mutex, then a queue_mutex).
  if (int rc = bind(dec->ctx)) return rc;
  if (int rc = flush_stream(dec->ctx, s, dec)) return rc;
  std::lock_guard<std::mutex> lock(dec->queue_mutex);
  PendingQueue *q = nullptr;
  if (dec->coalesce_max_age_us > 0 && !capturing(s)) {  // this decoder's queues of OTHER streams that have waited too long (never from inside a capture)
    const int64_t limit = now_us() - dec->coalesce_max_age_us;
    for (PendingQueue &c : dec->queues)
      if (c.stream != s && !c.frames.empty() && c.oldest_us <= limit)
        if (int rc = issue_queue(dec, c)) return rc;
  }
  for (PendingQueue &c : dec->queues)
    if (c.stream == s) q = &c;
  const int n = dec->coalesce.load();  // read ONCE, behind the mutex: set_coalescing changes it under the same mutex
  // A planar CHW target is never queued (its rows are not 4-byte pixels: write_of / row_bytes_of below never see one); like any
  // call that is not eligible it goes out behind what is queued, in stream order.  A batch with a CHW surface anywhere in it is
  // decode_batch_now's to judge.
  bool chw = false;
  for (int i = 0; outs != nullptr && i < count; ++i) chw = chw || is_chw(outs[i].format);
  const bool eligible = n > 1 && wait_until_completed == 0 && count >= 1 && count < n && frames != nullptr && outs != nullptr && !chw;
  if (!eligible) {  // in stream order: what is queued goes first
    if (q != nullptr)
      if (int rc = issue_queue(dec, *q)) return rc;
    return decode_batch_now(dec, layout, count, frames, alphas, outs, stream, wait_until_completed);
  }
  {  // the call's own status: everything -decodeBT709: checks, now
    DecodeParams p;
    BatchInfo info;
    if (int rc = gather_batch(dec, count, frames, alphas, outs, OutShape::kSame, layout, stream, &p, &info)) return rc;
    if (layout == BT709HIP_CHROMA_I420 && info.format == BT709HIP_FORMAT_RGBA16F) return BT709HIP_ERR_UNSUPPORTED;  // decode_batch_now's refusal, now
    if (dec->composite_over != BT709HIP_OVER_OFF && info.format == BT709HIP_FORMAT_RGBA16F) return BT709HIP_ERR_UNSUPPORTED;  // BT709HIP_OPT_COMPOSITE_OVER's
    if (dec->unpremultiply != 0 && (info.format == BT709HIP_FORMAT_RGBA16F || dec->composite_over != BT709HIP_OVER_OFF)) return BT709HIP_ERR_UNSUPPORTED;  // and BT709HIP_OPT_UNPREMULTIPLY's
    if (p.width == 0) return BT709HIP_OK;  // empty frames: nothing to launch
  }
  if (q == nullptr) {
    dec->queues.emplace_back();
    q = &dec->queues.back();
    q->stream = s;
  }
  // the bytes this call writes and reads, as one range each: the queue keeps the union of its calls' and only a call that
  // touches that union is compared item by item
  const bt709hip_frame *read_alphas = dec->has_alpha ? alphas : nullptr;
  ByteSpan writes, reads;
  for (int i = 0; i < count; ++i) {
    join(writes, write_of(outs[i]));
    const ItemReads r = reads_of(frames[i], read_alphas ? &read_alphas[i] : nullptr, layout);
    for (const ByteSpan &pl : r.plane) join(reads, pl);
  }
  if (!q->frames.empty()) {
    const bool fits = q->frames.size() + static_cast<size_t>(count) <= static_cast<size_t>(n) &&
                      same_shape(q->frames[0], frames[0]) && q->frames[0].transfer == frames[0].transfer &&
                      q->outs[0].stride == outs[0].stride && q->outs[0].format == outs[0].format && q->layout == layout &&
                      q->with_alphas == (alphas != nullptr) && (alphas == nullptr || q->alphas[0].y_stride == alphas[0].y_stride);
    if (!fits || conflicts(*q, writes, reads, count, frames, read_alphas, outs))
      if (int rc = issue_queue(dec, *q)) return rc;
  }
  q->with_alphas = alphas != nullptr;
  q->layout = layout;
  if (q->frames.empty()) {
    q->oldest_us = now_us();
    q->writes = q->reads = ByteSpan{};
  }
  join(q->writes, writes);
  join(q->reads, reads);
  q->frames.insert(q->frames.end(), frames, frames + count);
  if (alphas != nullptr) q->alphas.insert(q->alphas.end(), alphas, alphas + count);
  q->outs.insert(q->outs.end(), outs, outs + count);
  set_kernel_name("(queued: coalescing submit)");
  if (q->frames.size() >= static_cast<size_t>(n)) return issue_queue(dec, *q);
  return BT709HIP_OK;
}

}  // namespace bt709shim

extern "C" {

int bt709hip_decoder_flush(bt709hip_decoder *dec, void *stream) {
  if (dec == nullptr) return BT709HIP_ERR_INVALID_ARG;
  if (dec->ctx == nullptr) return BT709HIP_OK;  // never had a stream to queue on
  if (int rc = bind(dec->ctx)) return rc;
  return flush_decoder(dec, pick(dec->ctx, stream), false);
}

int bt709hip_decoder_flush_all(bt709hip_decoder *dec) {
  if (dec == nullptr) return BT709HIP_ERR_INVALID_ARG;
  if (dec->ctx == nullptr) return BT709HIP_OK;
  if (int rc = bind(dec->ctx)) return rc;
  return flush_decoder(dec, nullptr, true);
}

}  // extern "C"
