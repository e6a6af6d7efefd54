// batch_internal.h -- batched independent fits: what batch_data.cpp (the batch a context holds) and batch_calls.cpp (what is done
// with it) share.  Nothing else of either crosses a file boundary but the C ABI; their generated kernels live in the context's kernel
// cache, their one static kernel in frames.hip (kernels.h) and their blocks in gfh_ctx::batch (context.h).
#pragma once
#include "context_internal.h"

namespace gfh {

// batch_data.cpp
int check_context(gfh_ctx* c, const char* who);      // what a batch cannot be on: refused with or without a GPU
int data_form(const gfh_ctx* c);                     // 0 ragged, 1 ... 15 a cube by sample type and weight rule

}  // namespace gfh
