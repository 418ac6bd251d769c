// Python bindings for the gfx950 kernel set (hyperspot._C).
//
// Host-side glue only — every kernel lives in a .hip translation unit and
// is reached through a plain launcher so this file needs no device code.
#include <torch/extension.h>

#include <c10/hip/HIPStream.h>
#include <hip/hip_bf16.h>

#include <stdexcept>

using bf16 = __hip_bfloat16;

void launch_rmsnorm(bf16*, const bf16*, const bf16*, float, long, int,
                    hipStream_t);
void launch_fused_add_rmsnorm(bf16*, bf16*, const bf16*, float, long, int,
                              hipStream_t);
void launch_rope_kv_append(bf16*, bf16*, const bf16*, const long*,
                           const float*, const long*, bf16*, bf16*, long,
                           int, int, int, int, long, long, long, bool,
                           hipStream_t);
void launch_paged_attn(bf16*, const bf16*, const bf16*, const bf16*,
                       const int*, const int*, const int*, long, int, int,
                       int, int, int, float, long, float*, int, bool,
                       hipStream_t);
void launch_attn_prefill_mfma(bf16*, const bf16*, const bf16*,
                              const bf16*, const int*, int, int, int, int,
                              int, float, long, long, long, hipStream_t);
void launch_attn_prefill_paged_mfma(bf16*, const bf16*, const bf16*,
                                    const bf16*, const int*, const int*,
                                    const int*, int, int, int, int, int, int,
                                    int, float, long, bool, hipStream_t);
void launch_silu_mul(bf16*, const bf16*, long, int, hipStream_t);
void launch_quant_fp8(unsigned char*, float*, const bf16*, long, int, long,
                      hipStream_t);
void launch_fused_add_rmsnorm_fp8(unsigned char*, float*, const bf16*,
                                  bf16*, const bf16*, float, long, int,
                                  hipStream_t);
void launch_silu_mul_fp8(unsigned char*, float*, const bf16*, long, int,
                         hipStream_t);
void launch_moe_align(int*, int*, int*, const int*, int, int, int,
                      hipStream_t);
void launch_moe_gemm(bf16*, float*, const bf16*, const bf16*, const int*,
                     const int*, int, int, int, int, int, hipStream_t);
void launch_moe_combine(bf16*, const bf16*, const float*, const int*, long,
                        int, int, hipStream_t);
void launch_moe_gemm_fp8(bf16*, float*, const unsigned char*, const float*,
                         const unsigned char*, const float*, const int*,
                         const int*, int, int, int, int, int, hipStream_t);
void launch_greedy_sample(long*, const bf16*, long, int, hipStream_t);
void launch_inv_cdf_sample(long*, const float*, const float*, long, int,
                           hipStream_t);
void launch_sample_fused(long*, const bf16*, const float*, const float*,
                         const int*, const float*, long, int, hipStream_t);
void launch_token_logprobs(float*, int*, const bf16*, const long*, const int*,
                           long, int, hipStream_t);
void launch_decode_advance(long*, long*, int*, long*, int*, const long*,
                           const int*, int, int, int, hipStream_t);
void launch_penalty_build(int*, const int*, const int*, const int*,
                          const int*, int, int, int, int, hipStream_t);
void launch_penalty_apply(bf16*, const int*, const float*, const float*,
                          const float*, const int*, long, int, int,
                          hipStream_t);
void launch_penalty_note(int*, const int*, const long*, long, int, int,
                         hipStream_t);
int guided_words();
void launch_guided_json_mask(bf16*, const int*, long, int, hipStream_t);
void launch_guided_json_advance(int*, const long*, long, hipStream_t);

namespace {

hipStream_t stream() {
  return c10::hip::getCurrentHIPStream().stream();
}

void check(const torch::Tensor& t, torch::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
  TORCH_CHECK(t.scalar_type() == dt, name, " has wrong dtype");
}

bf16* bf(torch::Tensor& t) { return reinterpret_cast<bf16*>(t.data_ptr()); }
const bf16* cbf(const torch::Tensor& t) {
  return reinterpret_cast<const bf16*>(t.data_ptr());
}

void rmsnorm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
             double eps) {
  check(out, torch::kBFloat16, "out");
  check(x, torch::kBFloat16, "x");
  check(w, torch::kBFloat16, "w");
  const int hidden = (int)x.size(-1);
  TORCH_CHECK(hidden % 8 == 0 && hidden <= 16384, "hidden size");
  launch_rmsnorm(bf(out), cbf(x), cbf(w), (float)eps, x.numel() / hidden,
                 hidden, stream());
}

void fused_add_rmsnorm(torch::Tensor x, torch::Tensor residual,
                       torch::Tensor w, double eps) {
  check(x, torch::kBFloat16, "x");
  check(residual, torch::kBFloat16, "residual");
  const int hidden = (int)x.size(-1);
  TORCH_CHECK(hidden % 8 == 0 && hidden <= 16384, "hidden size");
  launch_fused_add_rmsnorm(bf(x), bf(residual), cbf(w), (float)eps,
                           x.numel() / hidden, hidden, stream());
}

// q/k/v may be strided views into one fused qkv buffer: require only the
// head dim contiguous (stride(2)==1) and head stride == D.
void check_qkv_view(const torch::Tensor& t, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be on GPU");
  TORCH_CHECK(t.scalar_type() == torch::kBFloat16, name, " must be bf16");
  TORCH_CHECK(t.dim() == 3 && t.stride(2) == 1 &&
                  t.stride(1) == t.size(2),
              name, " must be [T, H, D] with contiguous heads");
}

void rope_kv_append(torch::Tensor q, torch::Tensor k, torch::Tensor v,
                    torch::Tensor positions, torch::Tensor cos_sin,
                    torch::Tensor slot_mapping, torch::Tensor k_cache,
                    torch::Tensor v_cache) {
  check_qkv_view(q, "q");
  check_qkv_view(k, "k");
  check_qkv_view(v, "v");
  check(cos_sin, torch::kFloat32, "cos_sin");
  check(positions, torch::kInt64, "positions");
  check(slot_mapping, torch::kInt64, "slot_mapping");
  const long T = q.size(0);
  const int H = (int)q.size(1), KV = (int)k.size(1), D = (int)q.size(2);
  const int BS = (int)k_cache.size(2);
  const bool kv_fp8 =
      k_cache.scalar_type() == torch::kFloat8_e4m3fn;
  launch_rope_kv_append(bf(q), bf(k), cbf(v),
                        positions.data_ptr<long>(),
                        cos_sin.data_ptr<float>(),
                        slot_mapping.data_ptr<long>(), bf(k_cache),
                        bf(v_cache), T, H, KV, D, BS, q.stride(0),
                        k.stride(0), v.stride(0), kv_fp8, stream());
}

void paged_attn(torch::Tensor out, torch::Tensor q, torch::Tensor k_cache,
                torch::Tensor v_cache, torch::Tensor block_tables,
                torch::Tensor ctx_lens,
                c10::optional<torch::Tensor> row_seq, double scale,
                c10::optional<torch::Tensor> split_ws, long split) {
  check(out, torch::kBFloat16, "out");
  check_qkv_view(q, "q");
  check(block_tables, torch::kInt32, "block_tables");
  check(ctx_lens, torch::kInt32, "ctx_lens");
  const long R = q.size(0);
  const int H = (int)q.size(1), D = (int)q.size(2);
  const int KV = (int)k_cache.size(1), BS = (int)k_cache.size(2);
  TORCH_CHECK(H % KV == 0, "GQA group");
  const int* rs = nullptr;
  if (row_seq.has_value()) {
    check(*row_seq, torch::kInt32, "row_seq");
    rs = row_seq->data_ptr<int>();
  }
  float* ws = nullptr;
  if (split > 1) {
    TORCH_CHECK(split_ws.has_value(), "split>1 needs a workspace");
    check(*split_ws, torch::kFloat, "split_ws");
    TORCH_CHECK(split_ws->numel() >= R * KV * split * (H / KV) * (D + 2),
                "split_ws too small");
    ws = split_ws->data_ptr<float>();
  }
  const bool kv_fp8 =
      k_cache.scalar_type() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type(),
              "k/v cache dtype mismatch");
  launch_paged_attn(bf(out), cbf(q), cbf(k_cache), cbf(v_cache),
                    block_tables.data_ptr<int>(), ctx_lens.data_ptr<int>(),
                    rs, R, KV, H / KV, D, (int)block_tables.size(1), BS,
                    (float)scale, q.stride(0), ws, (int)split, kv_fp8,
                    stream());
}

// What both MFMA prefill bindings ask of out, q, the kv head count,
// seq_start and max_seqlen.
void check_prefill_args(const torch::Tensor& out, const torch::Tensor& q,
                        int KV, const torch::Tensor& seq_start,
                        long max_seqlen) {
  check(out, torch::kBFloat16, "out");
  check_qkv_view(q, "q");
  TORCH_CHECK(out.dim() == 3 && out.sizes() == q.sizes(),
              "out must be [T, H, D] like q");
  const int H = (int)q.size(1);
  TORCH_CHECK(KV > 0 && H % KV == 0, "GQA group: H=", H,
              " is no multiple of KV=", KV);
  check(seq_start, torch::kInt32, "seq_start");
  TORCH_CHECK(seq_start.dim() == 1 && seq_start.numel() >= 1,
              "seq_start must be [S+1]");
  TORCH_CHECK(max_seqlen >= 0, "max_seqlen must be >= 0");
}

void attn_prefill_mfma(torch::Tensor out, torch::Tensor q, torch::Tensor k,
                       torch::Tensor v, torch::Tensor seq_start,
                       long max_seqlen, double scale) {
  check_qkv_view(k, "k");
  check_qkv_view(v, "v");
  const int KV = (int)k.size(1);
  check_prefill_args(out, q, KV, seq_start, max_seqlen);
  const int H = (int)q.size(1), D = (int)q.size(2);
  TORCH_CHECK(k.sizes() == v.sizes() && k.size(0) == q.size(0) &&
                  k.size(2) == D,
              "k/v must be [T, KV, D] with q's T and D, and equal-shaped");
  launch_attn_prefill_mfma(
      bf(out), cbf(q), cbf(k), cbf(v), seq_start.data_ptr<int>(),
      (int)seq_start.numel() - 1, (int)max_seqlen, H, KV, D, (float)scale,
      q.stride(0), k.stride(0), v.stride(0), stream());
}

// Flash prefill over the paged cache: sequence z owns q rows
// seq_start[z]..seq_start[z+1]-1 at positions ctx_start[z]+i.  Nothing here
// reads device data: the caller vouches that block_tables covers
// ceil((ctx_start[z] + n_z) / 16) pages per sequence.
void attn_prefill_paged_mfma(torch::Tensor out, torch::Tensor q,
                             torch::Tensor k_cache, torch::Tensor v_cache,
                             torch::Tensor block_tables,
                             torch::Tensor seq_start,
                             torch::Tensor ctx_start, long max_seqlen,
                             double scale) {
  TORCH_CHECK(k_cache.is_cuda() && v_cache.is_cuda() &&
                  k_cache.is_contiguous() && v_cache.is_contiguous(),
              "k_cache/v_cache must be contiguous GPU tensors");
  TORCH_CHECK(k_cache.dim() == 4 && k_cache.sizes() == v_cache.sizes(),
              "k_cache/v_cache must be [NB, KV, 16, 128] and equal-shaped");
  const int KV = (int)k_cache.size(1);
  check_prefill_args(out, q, KV, seq_start, max_seqlen);
  const int H = (int)q.size(1);
  TORCH_CHECK(q.size(2) == 128,
              "attn_prefill_paged_mfma: head_dim must be 128, got ",
              q.size(2));
  TORCH_CHECK(k_cache.size(2) == 16,
              "attn_prefill_paged_mfma: page size must be 16, got ",
              k_cache.size(2));
  TORCH_CHECK(k_cache.size(3) == 128, "cache head_dim must be 128, got ",
              k_cache.size(3));
  TORCH_CHECK(v_cache.scalar_type() == k_cache.scalar_type(),
              "k/v cache dtype mismatch");
  const bool kv_fp8 = k_cache.scalar_type() == torch::kFloat8_e4m3fn;
  TORCH_CHECK(kv_fp8 || k_cache.scalar_type() == torch::kBFloat16,
              "cache dtype must be bfloat16 or float8_e4m3fn");
  check(block_tables, torch::kInt32, "block_tables");
  check(ctx_start, torch::kInt32, "ctx_start");
  const int S = (int)seq_start.numel() - 1;
  TORCH_CHECK(ctx_start.dim() == 1 && ctx_start.numel() == S,
              "ctx_start must be [S] with S = seq_start.numel() - 1");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == S,
              "block_tables must be [S, max_blocks]");
  launch_attn_prefill_paged_mfma(
      bf(out), cbf(q), cbf(k_cache), cbf(v_cache),
      block_tables.data_ptr<int>(), seq_start.data_ptr<int>(),
      ctx_start.data_ptr<int>(), S, (int)max_seqlen, H, KV,
      (int)q.size(2), (int)block_tables.size(1), (int)k_cache.size(2),
      (float)scale, q.stride(0), kv_fp8, stream());
}

void silu_mul(torch::Tensor out, torch::Tensor x) {
  check(out, torch::kBFloat16, "out");
  check(x, torch::kBFloat16, "x");
  const int inter = (int)out.size(-1);
  TORCH_CHECK(x.size(-1) == 2 * inter && inter % 8 == 0, "shape");
  launch_silu_mul(bf(out), cbf(x), out.numel() / inter, inter, stream());
}

void greedy_sample(torch::Tensor out, torch::Tensor logits) {
  check(out, torch::kInt64, "out");
  check(logits, torch::kBFloat16, "logits");
  launch_greedy_sample(out.data_ptr<long>(), cbf(logits), logits.size(0),
                       (int)logits.size(1), stream());
}

void inv_cdf_sample(torch::Tensor out, torch::Tensor logits,
                    torch::Tensor uniform) {
  check(out, torch::kInt64, "out");
  check(logits, torch::kFloat32, "logits");
  check(uniform, torch::kFloat32, "uniform");
  launch_inv_cdf_sample(out.data_ptr<long>(), logits.data_ptr<float>(),
                        uniform.data_ptr<float>(), logits.size(0),
                        (int)logits.size(1), stream());
}

void sample_fused(torch::Tensor out, torch::Tensor logits,
                  torch::Tensor temperature, torch::Tensor top_p,
                  torch::Tensor top_k, torch::Tensor uniform) {
  check(out, torch::kInt64, "out");
  check(logits, torch::kBFloat16, "logits");
  check(temperature, torch::kFloat32, "temperature");
  check(top_p, torch::kFloat32, "top_p");
  check(top_k, torch::kInt32, "top_k");
  check(uniform, torch::kFloat32, "uniform");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) > 0,
              "logits must be [rows, vocab]");
  const int64_t rows = logits.size(0);
  TORCH_CHECK(logits.size(1) < (1LL << 30), "vocab too large");
  TORCH_CHECK(out.numel() == rows && temperature.numel() == rows &&
                  top_p.numel() == rows && top_k.numel() == rows &&
                  uniform.numel() == rows,
              "per-row tensors must have `rows` elements");
  for (const torch::Tensor* t : {&out, &temperature, &top_p, &top_k, &uniform})
    TORCH_CHECK(t->device() == logits.device(),
                "sample_fused: tensors on different devices");
  launch_sample_fused(out.data_ptr<long>(), cbf(logits),
                      temperature.data_ptr<float>(), top_p.data_ptr<float>(),
                      top_k.data_ptr<int>(), uniform.data_ptr<float>(), rows,
                      (int)logits.size(1), stream());
}

// Chosen-token logprob and the n_top[r] most likely alternatives per row
// (csrc/logprobs.hip).  n_top[r] < 0 leaves row r of the outputs untouched;
// the contract is 0..20, larger values are clamped to 20 by the kernel.
void token_logprobs(torch::Tensor out_val, torch::Tensor out_id,
                    torch::Tensor logits, torch::Tensor chosen,
                    torch::Tensor n_top) {
  check(out_val, torch::kFloat32, "out_val");
  check(out_id, torch::kInt32, "out_id");
  check(logits, torch::kBFloat16, "logits");
  check(chosen, torch::kInt64, "chosen");
  check(n_top, torch::kInt32, "n_top");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) > 0,
              "logits must be [rows, vocab]");
  const int64_t rows = logits.size(0);
  TORCH_CHECK(logits.size(1) < (1LL << 30), "vocab too large");
  TORCH_CHECK(out_val.dim() == 2 && out_val.size(0) == rows &&
                  out_val.size(1) == 21 && out_id.dim() == 2 &&
                  out_id.size(0) == rows && out_id.size(1) == 21,
              "out_val / out_id must be [rows, 21]");
  TORCH_CHECK(chosen.numel() == rows && n_top.numel() == rows,
              "per-row tensors must have `rows` elements");
  for (const torch::Tensor* t : {&out_val, &out_id, &chosen, &n_top})
    TORCH_CHECK(t->device() == logits.device(),
                "token_logprobs: tensors on different devices");
  launch_token_logprobs(out_val.data_ptr<float>(), out_id.data_ptr<int>(),
                        cbf(logits), chosen.data_ptr<long>(),
                        n_top.data_ptr<int>(), rows, (int)logits.size(1),
                        stream());
}

void decode_advance(torch::Tensor input_ids, torch::Tensor positions,
                    torch::Tensor seq_lens, torch::Tensor slot_mapping,
                    torch::Tensor block_tables, torch::Tensor sampled_prev,
                    torch::Tensor ctl, int64_t page) {
  check(input_ids, torch::kInt64, "input_ids");
  check(positions, torch::kInt64, "positions");
  check(seq_lens, torch::kInt32, "seq_lens");
  check(slot_mapping, torch::kInt64, "slot_mapping");
  check(block_tables, torch::kInt32, "block_tables");
  check(sampled_prev, torch::kInt64, "sampled_prev");
  check(ctl, torch::kInt32, "ctl");
  const int64_t rows = input_ids.numel();
  TORCH_CHECK(rows > 0 && page > 0, "empty decode_advance");
  TORCH_CHECK(block_tables.dim() == 2 && block_tables.size(0) == rows,
              "block_tables must be [rows, max_blocks]");
  TORCH_CHECK(positions.numel() == rows && seq_lens.numel() == rows &&
                  slot_mapping.numel() == rows &&
                  sampled_prev.numel() == rows,
              "per-row tensors must have `rows` elements");
  TORCH_CHECK(ctl.numel() >= 4 * rows + 1, "ctl must hold 4*rows+1 ints");
  launch_decode_advance(input_ids.data_ptr<long>(), positions.data_ptr<long>(),
                        seq_lens.data_ptr<int>(),
                        slot_mapping.data_ptr<long>(),
                        block_tables.data_ptr<int>(),
                        sampled_prev.data_ptr<long>(), ctl.data_ptr<int>(),
                        (int)rows, (int)block_tables.size(1), (int)page,
                        stream());
}

// Penalty state (csrc/penalties.hip): table int32 [slots, vocab], word =
// 2 * count among generated tokens + (token occurs in the prompt).
void check_penalty_table(const torch::Tensor& table) {
  check(table, torch::kInt32, "table");
  TORCH_CHECK(table.dim() == 2 && table.size(0) > 0 && table.size(1) > 0,
              "table must be int32 [slots, vocab]");
  TORCH_CHECK(table.size(0) < (1LL << 30) && table.size(1) < (1LL << 30),
              "table too large");
}

// Row slots[i] of the table := history tokens[offsets[i]:offsets[i+1]], the
// first prompt_len[i] of them prompt.  Not for capture (the grid is n).
void penalty_build(torch::Tensor table, torch::Tensor slots,
                   torch::Tensor tokens, torch::Tensor offsets,
                   torch::Tensor prompt_len) {
  check_penalty_table(table);
  check(slots, torch::kInt32, "slots");
  check(tokens, torch::kInt32, "tokens");
  check(offsets, torch::kInt32, "offsets");
  check(prompt_len, torch::kInt32, "prompt_len");
  const int64_t n = slots.numel();
  TORCH_CHECK(offsets.numel() == n + 1 && prompt_len.numel() == n,
              "penalty_build: offsets must hold n + 1, prompt_len n entries");
  TORCH_CHECK(tokens.numel() < (1LL << 31), "too many history tokens");
  for (const torch::Tensor* t : {&slots, &tokens, &offsets, &prompt_len})
    TORCH_CHECK(t->device() == table.device(),
                "penalty_build: tensors on different devices");
  launch_penalty_build(table.data_ptr<int>(), slots.data_ptr<int>(),
                       tokens.data_ptr<int>(), offsets.data_ptr<int>(),
                       prompt_len.data_ptr<int>(), (int)n,
                       (int)table.size(0), (int)table.size(1),
                       (int)tokens.numel(), stream());
}

// In place on logits [rows, vocab]; rows with slot < 0 are left alone.
void penalty_apply(torch::Tensor logits, torch::Tensor slot,
                   torch::Tensor rep, torch::Tensor pres, torch::Tensor freq,
                   torch::Tensor table) {
  check_penalty_table(table);
  check(logits, torch::kBFloat16, "logits");
  check(slot, torch::kInt32, "slot");
  check(rep, torch::kFloat32, "rep");
  check(pres, torch::kFloat32, "pres");
  check(freq, torch::kFloat32, "freq");
  TORCH_CHECK(logits.dim() == 2 && logits.size(1) == table.size(1),
              "logits must be [rows, vocab] with the table's vocab");
  const int64_t rows = logits.size(0);
  // the grid is rows * chunks of 8192 logits
  TORCH_CHECK(rows * (table.size(1) / 8192 + 2) < (1LL << 31),
              "rows * vocab too large");
  TORCH_CHECK(slot.numel() >= rows && rep.numel() >= rows &&
                  pres.numel() >= rows && freq.numel() >= rows,
              "per-row tensors must have at least `rows` elements");
  for (const torch::Tensor* t : {&slot, &rep, &pres, &freq, &table})
    TORCH_CHECK(t->device() == logits.device(),
                "penalty_apply: tensors on different devices");
  launch_penalty_apply(bf(logits), slot.data_ptr<int>(),
                       rep.data_ptr<float>(), pres.data_ptr<float>(),
                       freq.data_ptr<float>(), table.data_ptr<int>(), rows,
                       (int)table.size(0), (int)table.size(1), stream());
}

// table[slot[r], sampled[r]] += 2 for the first `rows` = sampled.numel()
// rows with slot >= 0 and a token inside the vocabulary.
void penalty_note(torch::Tensor table, torch::Tensor slot,
                  torch::Tensor sampled) {
  check_penalty_table(table);
  check(slot, torch::kInt32, "slot");
  check(sampled, torch::kInt64, "sampled");
  const int64_t rows = sampled.numel();
  TORCH_CHECK(slot.numel() >= rows,
              "slot must have at least `rows` elements");
  TORCH_CHECK(slot.device() == table.device() &&
                  sampled.device() == table.device(),
              "penalty_note: tensors on different devices");
  launch_penalty_note(table.data_ptr<int>(), slot.data_ptr<int>(),
                      sampled.data_ptr<long>(), rows, (int)table.size(0),
                      (int)table.size(1), stream());
}

// JSON-mode guided decoding (csrc/guided.hip): state int32 [rows, words],
// word 0 < 0 = not a guided row.
void check_guided_state(const torch::Tensor& state) {
  check(state, torch::kInt32, "state");
  TORCH_CHECK(state.dim() == 2 && state.size(1) == guided_words(),
              "state must be int32 [rows, ", guided_words(), "]");
}

// In place on logits [rows, vocab]: -inf on every token a guided row's state
// does not allow; rows with state[r, 0] < 0 are left alone.
void guided_json_mask(torch::Tensor logits, torch::Tensor state) {
  check(logits, torch::kBFloat16, "logits");
  check_guided_state(state);
  TORCH_CHECK(logits.dim() == 2, "logits must be [rows, vocab]");
  TORCH_CHECK(logits.size(1) >= 260,
              "guided_json_mask: the vocabulary must hold the 260 ids of "
              "the byte tokenizer, got ", logits.size(1));
  const int64_t rows = logits.size(0);
  TORCH_CHECK(logits.size(1) < (1LL << 31) - 8192 &&
                  rows * (logits.size(1) / 8192 + 2) < (1LL << 31),
              "rows * vocab too large");
  TORCH_CHECK(state.size(0) >= rows,
              "state must have at least `rows` rows");
  TORCH_CHECK(state.device() == logits.device(),
              "guided_json_mask: tensors on different devices");
  launch_guided_json_mask(bf(logits), state.data_ptr<int>(), rows,
                          (int)logits.size(1), stream());
}

// state[r] := state[r] fed sampled[r], for the first `rows` = sampled.numel()
// rows that are guided; tokens outside 4..259 are ignored.
void guided_json_advance(torch::Tensor state, torch::Tensor sampled) {
  check_guided_state(state);
  check(sampled, torch::kInt64, "sampled");
  const int64_t rows = sampled.numel();
  TORCH_CHECK(state.size(0) >= rows && rows < (1LL << 31),
              "state must have at least `rows` rows");
  TORCH_CHECK(sampled.device() == state.device(),
              "guided_json_advance: tensors on different devices");
  launch_guided_json_advance(state.data_ptr<int>(),
                             sampled.data_ptr<long>(), rows, stream());
}

}  // namespace


unsigned char* u8(torch::Tensor& t) {
  return reinterpret_cast<unsigned char*>(t.data_ptr());
}

void quant_fp8(torch::Tensor out, torch::Tensor scales, torch::Tensor x) {
  check(out, torch::kFloat8_e4m3fn, "out");
  check(scales, torch::kFloat, "scales");
  TORCH_CHECK(x.is_cuda() && x.scalar_type() == torch::kBFloat16, "x");
  const int hidden = (int)x.size(-1);
  TORCH_CHECK(x.stride(-1) == 1, "x inner dim must be contiguous");
  const long rows = x.numel() / hidden;
  const long stride = x.dim() > 1 ? x.stride(0) : hidden;
  launch_quant_fp8(u8(out), scales.data_ptr<float>(), cbf(x), rows, hidden,
                   stride, stream());
}

void fused_add_rmsnorm_fp8(torch::Tensor out, torch::Tensor scales,
                           torch::Tensor x, torch::Tensor residual,
                           torch::Tensor w, double eps) {
  check(out, torch::kFloat8_e4m3fn, "out");
  check(scales, torch::kFloat, "scales");
  check(x, torch::kBFloat16, "x");
  check(residual, torch::kBFloat16, "residual");
  check(w, torch::kBFloat16, "w");
  const int hidden = (int)x.size(-1);
  launch_fused_add_rmsnorm_fp8(u8(out), scales.data_ptr<float>(), cbf(x),
                               bf(residual), cbf(w), (float)eps,
                               x.numel() / hidden, hidden, stream());
}

void silu_mul_fp8(torch::Tensor out, torch::Tensor scales, torch::Tensor x) {
  check(out, torch::kFloat8_e4m3fn, "out");
  check(scales, torch::kFloat, "scales");
  check(x, torch::kBFloat16, "x");
  const int inter = (int)out.size(-1);
  TORCH_CHECK(x.size(-1) == 2 * inter, "x must be [rows, 2*inter]");
  launch_silu_mul_fp8(u8(out), scales.data_ptr<float>(), cbf(x),
                      out.numel() / inter, inter, stream());
}


constexpr long kMoeBM = 256;  // MOE_BM in csrc/moe.hip

// shape contract shared by the bf16 and fp8 grouped GEMMs: x [rows, K],
// w [E, N, K], out [ntiles*256, N], sorted_ids [ntiles*256]
void check_moe_gemm_shapes(const torch::Tensor& out, const torch::Tensor& x,
                           const torch::Tensor& w,
                           const torch::Tensor& sorted_ids,
                           const torch::Tensor& tile_expert,
                           long gather_div, const char* op) {
  const long P = tile_expert.numel() * kMoeBM;
  TORCH_CHECK(w.dim() == 3, op, ": w must be [E, N, K]");
  TORCH_CHECK(gather_div >= 0, op, ": gather_div must be >= 0");
  TORCH_CHECK(out.dim() == 2 && out.size(0) == P &&
                  out.size(1) == w.size(1),
              op, ": out must be [ntiles*256, N]");
  TORCH_CHECK(sorted_ids.numel() == P, op,
              ": sorted_ids must hold ntiles*256 entries");
  TORCH_CHECK(x.dim() == 2 && x.size(1) == w.size(2), op,
              ": x must be [rows, K]");
  if (gather_div == 0) {
    TORCH_CHECK(x.size(0) == P, op,
                ": plain mode needs x with ntiles*256 rows");
  } else {  // pad rows stage row 0 of x
    TORCH_CHECK(x.size(0) >= 1, op, ": gather mode needs a non-empty x");
  }
}

void moe_align(torch::Tensor sorted_ids, torch::Tensor tile_expert,
               torch::Tensor inv_pos, torch::Tensor flat_ids,
               long num_experts) {
  check(sorted_ids, torch::kInt, "sorted_ids");
  check(tile_expert, torch::kInt, "tile_expert");
  check(inv_pos, torch::kInt, "inv_pos");
  check(flat_ids, torch::kInt, "flat_ids");
  // everything the kernel (and the GEMMs after it) will use as an index
  // bound is settled here, on the host, without a sync
  TORCH_CHECK(num_experts >= 1 && num_experts <= 64,
              "moe_align: num_experts must be in [1, 64]");
  TORCH_CHECK(sorted_ids.numel() == tile_expert.numel() * kMoeBM,
              "moe_align: sorted_ids must hold ntiles*256 entries");
  TORCH_CHECK(tile_expert.numel() * kMoeBM >=
                  flat_ids.numel() + num_experts * (kMoeBM - 1),
              "moe_align: ntiles cannot hold the worst-case padded length");
  TORCH_CHECK(inv_pos.numel() == flat_ids.numel(),
              "moe_align: inv_pos must hold one entry per pair");
  launch_moe_align(sorted_ids.data_ptr<int>(), tile_expert.data_ptr<int>(),
                   inv_pos.data_ptr<int>(), flat_ids.data_ptr<int>(),
                   (int)flat_ids.numel(), (int)num_experts,
                   (int)tile_expert.numel(), stream());
}

void moe_gemm(torch::Tensor out, torch::Tensor x, torch::Tensor w,
              torch::Tensor sorted_ids, torch::Tensor tile_expert,
              long gather_div, long splitk,
              c10::optional<torch::Tensor> ws) {
  check(out, torch::kBFloat16, "out");
  check(x, torch::kBFloat16, "x");
  check(w, torch::kBFloat16, "w");
  check(sorted_ids, torch::kInt, "sorted_ids");
  check(tile_expert, torch::kInt, "tile_expert");
  check_moe_gemm_shapes(out, x, w, sorted_ids, tile_expert, gather_div,
                        "moe_gemm");
  float* wsp = nullptr;
  if (splitk > 1) {
    TORCH_CHECK(ws.has_value(), "moe_gemm: splitk>1 needs a workspace");
    check(*ws, torch::kFloat, "ws");
    TORCH_CHECK(ws->numel() >= splitk * out.numel(),
                "moe_gemm: workspace too small");
    wsp = ws->data_ptr<float>();
  }
  launch_moe_gemm(bf(out), wsp, cbf(x), cbf(w),
                  sorted_ids.data_ptr<int>(),
                  tile_expert.data_ptr<int>(), (int)tile_expert.numel(),
                  (int)w.size(1), (int)w.size(2), (int)gather_div,
                  (int)splitk, stream());
}

void moe_combine(torch::Tensor out, torch::Tensor y, torch::Tensor wts,
                 torch::Tensor inv_pos, long topk) {
  check(out, torch::kBFloat16, "out");
  check(y, torch::kBFloat16, "y");
  check(wts, torch::kFloat, "wts");
  check(inv_pos, torch::kInt, "inv_pos");
  TORCH_CHECK(topk >= 1, "moe_combine: topk must be >= 1");
  TORCH_CHECK(out.dim() == 2 && y.dim() == 2 && y.size(1) == out.size(1),
              "moe_combine: y and out must share the hidden size");
  TORCH_CHECK(wts.numel() == out.size(0) * topk &&
                  inv_pos.numel() == out.size(0) * topk,
              "moe_combine: wts and inv_pos must hold T*topk entries");
  if (out.size(0) == 0) return;  // a rank that received nothing: no grid
  launch_moe_combine(bf(out), cbf(y), wts.data_ptr<float>(),
                     inv_pos.data_ptr<int>(), out.size(0), (int)topk,
                     (int)out.size(-1), stream());
}


void moe_gemm_fp8(torch::Tensor out, torch::Tensor xq, torch::Tensor xs,
                  torch::Tensor wq, torch::Tensor ws,
                  torch::Tensor sorted_ids, torch::Tensor tile_expert,
                  long gather_div, long splitk,
                  c10::optional<torch::Tensor> skw) {
  check(out, torch::kBFloat16, "out");
  check(xq, torch::kFloat8_e4m3fn, "xq");
  check(xs, torch::kFloat, "xs");
  check(wq, torch::kFloat8_e4m3fn, "wq");
  check(ws, torch::kFloat, "ws");
  check(sorted_ids, torch::kInt, "sorted_ids");
  check(tile_expert, torch::kInt, "tile_expert");
  check_moe_gemm_shapes(out, xq, wq, sorted_ids, tile_expert, gather_div,
                        "moe_gemm_fp8");
  TORCH_CHECK(xs.numel() == xq.size(0),
              "moe_gemm_fp8: xs must hold one scale per row of xq");
  TORCH_CHECK(ws.numel() == wq.size(0) * wq.size(1),
              "moe_gemm_fp8: ws must hold E*N scales");
  float* skp = nullptr;
  if (splitk > 1) {
    TORCH_CHECK(skw.has_value(),
                "moe_gemm_fp8: splitk>1 needs a workspace");
    check(*skw, torch::kFloat, "skw");
    TORCH_CHECK(skw->numel() >= splitk * out.numel(),
                "moe_gemm_fp8: workspace too small");
    skp = skw->data_ptr<float>();
  }
  launch_moe_gemm_fp8(bf(out), skp, u8(xq), xs.data_ptr<float>(), u8(wq),
                      ws.data_ptr<float>(), sorted_ids.data_ptr<int>(),
                      tile_expert.data_ptr<int>(),
                      (int)tile_expert.numel(), (int)wq.size(1),
                      (int)wq.size(2), (int)gather_div, (int)splitk,
                      stream());
}

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.doc() = "HyperSpot-AMD gfx950 (CDNA4) kernels";
  m.def("rmsnorm", &rmsnorm);
  m.def("quant_fp8", &quant_fp8);
  m.def("fused_add_rmsnorm_fp8", &fused_add_rmsnorm_fp8);
  m.def("silu_mul_fp8", &silu_mul_fp8);
  m.def("moe_align", &moe_align);
  m.def("moe_gemm", &moe_gemm);
  m.def("moe_combine", &moe_combine);
  m.def("moe_gemm_fp8", &moe_gemm_fp8);
  m.def("fused_add_rmsnorm", &fused_add_rmsnorm);
  m.def("rope_kv_append", &rope_kv_append);
  m.def("paged_attn", &paged_attn);
  m.def("attn_prefill_mfma", &attn_prefill_mfma);
  m.def("attn_prefill_paged_mfma", &attn_prefill_paged_mfma);
  m.def("silu_mul", &silu_mul);
  m.def("greedy_sample", &greedy_sample);
  m.def("inv_cdf_sample", &inv_cdf_sample);
  m.def("sample_fused", &sample_fused);
  m.def("token_logprobs", &token_logprobs);
  m.def("decode_advance", &decode_advance);
  m.def("penalty_build", &penalty_build);
  m.def("penalty_apply", &penalty_apply);
  m.def("penalty_note", &penalty_note);
  m.def("guided_json_mask", &guided_json_mask);
  m.def("guided_json_advance", &guided_json_advance);
}
