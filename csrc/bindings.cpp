// Schema definitions of the sftamd custom-op library. Implementations live next to their
// kernels (TORCH_LIBRARY_IMPL(sftamd, CUDA, ...) in each .hip file); the CPU path of every
// op is the PyTorch reference in llm_fine_tune_distributed_amd/ops/reference.py, except the
// native data-pipeline ops below which are CPU kernels.
#include <torch/library.h>

#include <string>
#include <vector>

namespace sftamd {
// csrc/ipc_allreduce.hip: one-shot peer-memory all-reduce for small messages
int64_t ipc_ar_create(int64_t cap, int64_t world, int64_t rank);
std::vector<int64_t> ipc_ar_handle(int64_t id);
void ipc_ar_open(int64_t id, std::vector<int64_t> handles);
int64_t ipc_ar_check(int64_t id);
int64_t ipc_ar_poll(int64_t id);
int64_t ipc_ar_uncached(int64_t id);
void ipc_ar_destroy(int64_t id);
// csrc/ddp_reducer.cpp: bucket planner + ready tracker of the DDP engine
std::vector<int64_t> ddp_plan(std::vector<int64_t> sizes, std::vector<int64_t> region, int64_t tied, int64_t align,
                              int64_t pad_unit, int64_t cap, int64_t first_cap, int64_t split_at);
int64_t ddp_tracker_create(std::vector<int64_t> owner_ptr, std::vector<int64_t> owners, int64_t n_buckets);
void ddp_tracker_reset(int64_t id);
std::vector<int64_t> ddp_tracker_mark(int64_t id, int64_t param);
std::vector<int64_t> ddp_tracker_drain(int64_t id);
std::vector<int64_t> ddp_tracker_pending(int64_t id);
void ddp_tracker_destroy(int64_t id);
// csrc/dispatch_trace.cpp
void dispatch_trace(bool on);
std::string dispatch_trace_read();
int64_t set_cu_budget(int64_t n);
}

TORCH_LIBRARY(sftamd, m) {
  // runtime: CU-restricted HIP stream for the optimizer's side stream (no tensor arguments: catch-all kernel)
  // runtime: IPC peer-memory all-reduce contexts (no tensor arguments: catch-all kernels)
  m.def("ipc_ar_create(int cap, int world, int rank) -> int", &sftamd::ipc_ar_create);
  m.def("ipc_ar_handle(int ctx) -> int[]", &sftamd::ipc_ar_handle);
  m.def("ipc_ar_open(int ctx, int[] handles) -> ()", &sftamd::ipc_ar_open);
  m.def("ipc_ar_check(int ctx) -> int", &sftamd::ipc_ar_check);
  m.def("ipc_ar_poll(int ctx) -> int", &sftamd::ipc_ar_poll);
  m.def("ipc_ar_uncached(int ctx) -> int", &sftamd::ipc_ar_uncached);
  m.def("ipc_ar_destroy(int ctx) -> ()", &sftamd::ipc_ar_destroy);
  // runtime: DDP bucket planner / ready tracker (CPU, no tensor arguments)
  m.def("ddp_plan(int[] sizes, int[] region, int tied, int align, int pad_unit, int cap, int first_cap, "
        "int split_at) -> int[]", &sftamd::ddp_plan);
  m.def("ddp_tracker_create(int[] owner_ptr, int[] owners, int n_buckets) -> int", &sftamd::ddp_tracker_create);
  m.def("ddp_tracker_reset(int id) -> ()", &sftamd::ddp_tracker_reset);
  m.def("ddp_tracker_mark(int id, int param) -> int[]", &sftamd::ddp_tracker_mark);
  m.def("ddp_tracker_drain(int id) -> int[]", &sftamd::ddp_tracker_drain);
  m.def("ddp_tracker_pending(int id) -> int[]", &sftamd::ddp_tracker_pending);
  m.def("ddp_tracker_destroy(int id) -> ()", &sftamd::ddp_tracker_destroy);
  m.def("ipc_ar_allreduce(Tensor(a!) x, int ctx, int round, int blocks=16) -> ()");
  // runtime: dispatch trace of the kernel variants launched (tests assert the default paths)
  m.def("dispatch_trace(bool on) -> ()", &sftamd::dispatch_trace);
  m.def("dispatch_trace_read() -> str", &sftamd::dispatch_trace_read);
  m.def("set_cu_budget(int n) -> int", &sftamd::set_cu_budget);
  // norms / elementwise
  m.def("rmsnorm_fwd(Tensor x, Tensor? residual, Tensor weight, float eps, int y_ld=0) -> (Tensor, Tensor, Tensor)");
  m.def("rmsnorm_bwd(Tensor dy, Tensor h, Tensor weight, Tensor rstd, Tensor? dres, Tensor(a!)? dw_out=None, bool accumulate=False) -> (Tensor, Tensor)");
  m.def("swiglu_fwd(Tensor gate_up) -> Tensor");
  m.def("cu_hog(Tensor(a!) sink, int blocks, float usec) -> ()");
  m.def("swiglu_bwd(Tensor dy, Tensor gate_up) -> Tensor");
  m.def("rope_(Tensor(a!) qkv, Tensor cos, Tensor sin, int n_q, int n_kv, int head_dim, bool inverse) -> ()");
  // per-head QK RMSNorm + RoPE, in place on the q|k columns of the packed qkv (csrc/qk_norm.hip); fwd returns the raw
  // q|k copy for the backward (empty with save_raw=False), bwd returns (dq_weight, dk_weight) in fp32
  m.def("qk_norm_rope_fwd(Tensor(a!) qkv, Tensor q_weight, Tensor k_weight, Tensor cos, Tensor sin, int n_q, int n_kv, int head_dim, float eps, bool save_raw=True) -> Tensor");
  m.def("qk_norm_rope_bwd(Tensor(a!) dqkv, Tensor qk_raw, Tensor q_weight, Tensor k_weight, Tensor cos, Tensor sin, int n_q, int n_kv, int head_dim, float eps) -> (Tensor, Tensor)");
  // q / k / v projection bias + RoPE, in place on the packed qkv (csrc/qkv_bias.hip; Qwen2): fwd adds bias [(n_q + 2
  // n_kv) * 128] and rotates the q|k columns; bwd un-rotates the q|k columns of dqkv and returns dbias in fp32
  m.def("qkv_bias_rope_fwd(Tensor(a!) qkv, Tensor bias, Tensor cos, Tensor sin, int n_q, int n_kv, int head_dim) -> ()");
  m.def("qkv_bias_rope_bwd(Tensor(a!) dqkv, Tensor cos, Tensor sin, int n_q, int n_kv, int head_dim) -> Tensor");
  m.def("embedding_fwd(Tensor ids, Tensor weight) -> Tensor");
  // NEFTune: the gather plus mag[m] * u(m * H + c, seed), u uniform in (-1, 1) from hash_u32 (csrc/elementwise.hip)
  m.def("embedding_noise_fwd(Tensor ids, Tensor weight, Tensor mag, int seed) -> Tensor");
  m.def("dropout_add(Tensor? a, Tensor b, float p, int seed) -> Tensor");
  m.def("lora_widen(Tensor x, int R, float p, int seed) -> (Tensor, Tensor)");
  m.def("lora_fwd(Tensor x, Tensor A, float s, float p, int seed, int ldX=0, bool save_xd=False, bool swiglu=False) -> (Tensor, Tensor)");
  m.def("lora_bwd_dx(Tensor base, Tensor dxa, Tensor A, float p, int seed, Tensor? gu=None) -> Tensor");
  m.def("lora_tsum(Tensor X, int K, Tensor S, float p, int seed) -> Tensor");
  m.def("lora_fwd_inplace(Tensor(a!) X, int K, Tensor A, float s, float p, int seed) -> ()");
  m.def("lora_dxa(Tensor dy, Tensor Bc, float s) -> Tensor");
  m.def("lora_dxa_blocks(Tensor dy, Tensor Bc, int[] o, int[] rows, int[] c, int r, float s) -> Tensor");
  m.def("lora_grad_out(Tensor sum, Tensor(a!)[] outs, int[] r0, int[] c0, bool tr, int[] accumulate) -> ()");
  m.def("lora_grad_out2(Tensor sa, Tensor(a!)[] oa, int[] ra, int[] ca, bool ta, int[] aa, Tensor sb, "
        "Tensor(b!)[] ob, int[] rb, int[] cb, bool tb, int[] ab) -> ()");
  m.def("copy2d_batch(Tensor desc, int max_elems) -> ()");
  m.def("embedding_bwd(Tensor dy, Tensor sorted_ids, Tensor perm, Tensor(a!) grad_weight) -> ()");
  // loss
  // label_smoothing e in [0, 1) (HF LabelSmoother) or loss_mode 1 = dft (TRL dft_loss); stats row 0 is the objective
  // temperature tau != 1: the NLL, lse, entropy and argmax bit of softmax(x / tau); the gradient written is softmax(x /
  // tau) - onehot, the chain rule's 1 / tau left to the caller's row weight (not with smoothing or dft)
  m.def("ce_fwd(Tensor(a!) logits, Tensor labels, Tensor inv_count, bool write_grad, float label_smoothing=0.0, int loss_mode=0, float temperature=1.0) -> Tensor");
  // knowledge distillation (csrc/distill.hip): TRL's generalized JSD of the student's against the teacher's logits
  // at temperature tau, beta 0 = KL(teacher || student), 1 = KL(student || teacher); stats [5, M] = (loss, student
  // lse, teacher lse, student argmax == label, student argmax == teacher argmax); write_grad leaves the gradient
  // over student_logits
  m.def("kd_fwd(Tensor(a!) student_logits, Tensor teacher_logits, Tensor labels, Tensor inv_count, bool write_grad, float beta, float temperature) -> Tensor");
  // offline distillation (csrc/distill_topk.hip): the k largest logits per row, value descending and equal values by
  // column ascending, as (int32 ids [M, k], fp32 log softmax(x / tau) there, the lse over the whole row); and the
  // forward KL of the student against such a truncated teacher: stats [5, M] = (loss, student lse, teacher mass kept,
  // student argmax == label, student argmax == ids[:, 0]); write_grad leaves the gradient over student_logits. The ids
  // of a row are distinct and in [0, vocab)
  m.def("teacher_topk(Tensor logits, int k, float temperature) -> (Tensor, Tensor)");
  m.def("kd_topk_fwd(Tensor(a!) student_logits, Tensor ids, Tensor logps, Tensor labels, Tensor inv_count, bool write_grad, float temperature) -> Tensor");
  // sequence-level objectives (csrc/preference.hip): logps[s] = -sum nll[cu[s] : cu[s + 1]]; rows of sequence s times
  // coef[s] * gscale (rows at or past cu[n_seqs]: 0; csrc/scale_rows.hip); DPO per-pair stats [5, P] = (loss, coef, reward_c, reward_r, delta)
  m.def("seq_logp_sum(Tensor nll, Tensor cu_seqlens, int n_seqs) -> Tensor");
  m.def("scale_rows_by_seq(Tensor x, Tensor coef, Tensor cu_seqlens, int n_seqs, Tensor gscale) -> Tensor");
  m.def("scale_rows_by_seq_(Tensor(a!) x, Tensor coef, Tensor cu_seqlens, int n_seqs, Tensor gscale) -> ()");
  m.def("dpo_pair_fwd(Tensor logps, Tensor ref_logps, Tensor inv_pairs, float beta) -> Tensor");
  // reward modelling (csrc/reward.hip): scores[s] = h[last row of segment s] . w in fp32 (an empty segment: +0); its
  // backward (dh bf16 [M, H]: g_s w on those rows, +0 elsewhere; dw fp32 [H]), the half not needed returned undefined;
  // per-pair stats [4, P] = (softplus(-z) + c (r_c + r_r)^2, d / d r_c, d / d r_r, z), z = r_c - r_r - margin
  m.def("seq_score_fwd(Tensor h, Tensor w, Tensor cu_seqlens, int n_seqs) -> Tensor");
  m.def("seq_score_bwd(Tensor g, Tensor h, Tensor w, Tensor cu_seqlens, int n_seqs, bool need_dh, bool need_dw) -> (Tensor, Tensor)");
  m.def("reward_pair_fwd(Tensor scores, Tensor? margins, Tensor inv_pairs, float center_coef) -> Tensor");
  // per-token policy objective (csrc/policy.hip; GRPO): rows [2, M] = (w l, w dl/dlogp) per completion row (labels >=
  // 0), seq [6, S] = per-sequence sums (loss, completion tokens, low-clipped, high-clipped, KL, ratio); scale_rows is
  // scale_rows_by_seq's kernel without the segment search (csrc/scale_rows.hip): out[t, :] = x[t, :] * (coef[t] * gscale)
  m.def("grpo_token_fwd(Tensor nll, Tensor? old_logps, Tensor? ref_logps, Tensor labels, Tensor adv, Tensor cu_seqlens, int n_seqs, Tensor inv_norm, float eps_low, float eps_high, float beta, bool per_seq_mean) -> (Tensor, Tensor)");
  m.def("scale_rows(Tensor x, Tensor coef, Tensor gscale) -> Tensor");
  m.def("scale_rows_(Tensor(a!) x, Tensor coef, Tensor gscale) -> ()");
  // attention (window > 0: causal sliding window, query i sees keys (i - window, i]; 0: none)
  m.def("flash_fwd(Tensor qkv, Tensor cu_seqlens, int max_seqlen, int n_q, int n_kv, int head_dim, float scale, bool causal, int window=0) -> (Tensor, Tensor)");
  m.def("flash_bwd(Tensor dout, Tensor qkv, Tensor out, Tensor lse, Tensor cu_seqlens, int max_seqlen, int n_q, int n_kv, int head_dim, float scale, bool causal, Tensor? delta=None, int window=0) -> Tensor");
  m.def("flash_bwd_rope(Tensor dout, Tensor qkv, Tensor out, Tensor lse, Tensor cu_seqlens, int max_seqlen, int n_q, int n_kv, int head_dim, float scale, bool causal, Tensor cos, Tensor sin, Tensor? delta=None, int window=0) -> Tensor");
  m.def("decode_attention(Tensor q, Tensor kcache, Tensor vcache, Tensor cache_len, int n_q, int n_kv, float scale, int window=0) -> Tensor");
  m.def("decode_attention_batched(Tensor qkv, Tensor(a!) kcache, Tensor(b!) vcache, Tensor lens, int n_q, int n_kv, float scale, int window=0) -> Tensor");
  // fused decode sampler: penalty -> temperature -> top-k -> top-p -> draw, device-resident state
  m.def("sample_token(Tensor logits, Tensor(a!) presence, Tensor(b!) state, Tensor(c!)? tok_out, Tensor(d!)? pos_out, Tensor(e!)? len_out, Tensor(f!)? log, float temperature, int top_k, float top_p, float repetition_penalty, bool do_sample, int seed) -> ()");
  m.def("sample_tokens(Tensor logits, Tensor(a!) presence, Tensor(b!) state, Tensor(c!)? tok_out, Tensor(d!)? pos_out, Tensor(e!)? len_out, Tensor(f!)? log, Tensor(g!) done, int eos_token_id, float temperature, int top_k, float top_p, float repetition_penalty, bool do_sample, int seed) -> ()");
  // the full-vocabulary draw (Gumbel-max over softmax(penalised logits / temperature), no top-k / top-p) for B rows,
  // with sample_tokens' state / outputs and the drawn token's log-probability in logp_log fp32 [B, cap]
  m.def("sample_tokens_full(Tensor logits, Tensor(a!) presence, Tensor(b!) state, Tensor(c!)? tok_out, Tensor(d!)? pos_out, Tensor(e!)? len_out, Tensor(f!)? log, Tensor(g!) logp_log, Tensor(h!) done, int eos_token_id, float temperature, float repetition_penalty, int seed) -> ()");
  // weight-gradient GEMM: out[N,K] (+)= dy[T,N]^T x[T,K]
  m.def("wgrad_gemm(Tensor(a!) out, Tensor dy, Tensor x, bool accumulate, int cfg=14, Tensor(b!)? norm=None) -> ()");
  m.def("wgrad_gemm_multi(Tensor(a!)[] outs, Tensor[] dys, Tensor[] xs, int[] accs, Tensor(b!)[] norms, int split_all=0, int split_left=0) -> ()");
  m.def("wgrad_gemm_pair(Tensor(a!) out0, Tensor dy0, Tensor x0, bool acc0, Tensor(b!)? norm0, Tensor(c!) out1, Tensor dy1, Tensor x1, bool acc1, Tensor(d!)? norm1, int split_all=0) -> ()");
  // input-gradient GEMM dX = dy w (w [K, N]), optional fused SwiGLU backward (csrc/gemm_dgrad.hip)
  m.def("dgrad_gemm(Tensor dy, Tensor w, Tensor? gate_up=None, int cfg=14) -> Tensor");
  m.def("dgrad_gemm_delta(Tensor dy, Tensor w, Tensor attn_out) -> (Tensor, Tensor)");
  // forward-layout GEMM C = a w^T with fused epilogues (csrc/gemm_tn.hip)
  m.def("gemm_tn(Tensor a, Tensor w, int cfg=11) -> Tensor");
  m.def("gemm_tn_swiglu(Tensor x, Tensor w_gate_up, int cfg=11) -> (Tensor, Tensor)");
  m.def("gemm_tn_rope(Tensor x, Tensor w, Tensor cos, Tensor sin, int rope_cols, int cfg=11) -> Tensor");
  // optimizer
  m.def("sumsq(Tensor x) -> Tensor");
  m.def("sumsq_chunks(Tensor x, Tensor chunks) -> Tensor");
  m.def("adamw_flat(Tensor(a!) param, Tensor grad, Tensor(b!)? master, Tensor(c!) exp_avg, Tensor(d!) exp_avg_sq, Tensor clip_coef, float lr, float beta1, float beta2, float eps, float weight_decay, float bc1, float bc2, int sr_seed=0, int sr_offset=0) -> ()");
  // native data pipeline (CPU)
  m.def("pack_sequences(Tensor tokens, Tensor offsets, Tensor order, int max_tokens, int pad_id, int pad_multiple) -> (Tensor, Tensor, Tensor, Tensor, Tensor)");
  m.def("pad_batch(Tensor tokens, Tensor offsets, Tensor order, int pad_id, int pad_multiple, int max_length) -> (Tensor, Tensor, Tensor)");
}
