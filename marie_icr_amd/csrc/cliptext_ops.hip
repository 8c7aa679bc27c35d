// cliptext_ops.hip — the row kernel the CLIP text tower has that the vision tower (clip_ops.hip) does not: the token + position
// embedding (a row_ops.h load, add and store).  (Its causal attention is attn_seq.hip.)
//
// Replaces, in transformers/models/clip/modeling_clip.py: CLIPTextEmbeddings.forward (the same arithmetic as clip/model.py:
// CLIP.encode_text's token_embedding + positional_embedding).
#include "igemm_common.h"
#include "row_ops.h"

namespace {

// ------------------------------------------------------------------------------------------------------- embedding
// h[seq][t] = table[ids[seq][t]] + pos[t], fp32, one wave per row, 16 bytes a lane
__global__ __launch_bounds__(256) void cliptext_embed_kernel(const float* __restrict__ table, const float* __restrict__ pos,
                                                             const int* __restrict__ ids, float* __restrict__ h, int rows,
                                                             int npad, int D) {
  const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
  if (row >= rows) return;
  float4v v[ROW_GROUPS];
  row_load(v, table + (size_t)ids[row] * D, D, lane);
  row_add(v, pos + (size_t)(row % npad) * D, D, lane);
  row_store<float>(v, h + (size_t)row * D, nullptr, D, lane);
}

}  // namespace

int mhip_launch_cliptext_embed(mhip_ctx* ctx, const float* table, const float* pos, const int* ids, float* h, int B, int npad, int D) {
  if (B <= 0 || npad < 1 || !row_width_ok(D)) return mhip_fail(ctx, MHIP_EINVAL, "cliptext_embed: B=%d npad=%d D=%d", B, npad, D);
  const int rows = B * npad;
  PROF_LAUNCH(ctx, MHIP_K_CLIPTEXT_EMBED, hipLaunchKernelGGL(cliptext_embed_kernel, dim3((rows + 3) / 4), dim3(256), 0, ctx->stream, table, pos, ids, h, rows, npad, D));
  CHECK_LAUNCH(ctx, "cliptext_embed");
  return 0;
}
