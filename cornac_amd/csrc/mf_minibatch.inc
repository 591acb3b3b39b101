// MF minibatch path with dense optimisers — included at the end of mf.hip.
//
// Reference: cornac/models/mf/backend_pt.py:29-106 (`MF(backend="pytorch")`): per batch of `batch_size`
// ratings from `uir_iter(shuffle=True)`, pred = <U_u, V_i> (+ Bu_u + Bi_i + mu), loss = sum (pred - r)^2,
// autograd, then a torch.optim step {SGD, Adam, RMSprop, Adagrad}(lr, weight_decay = lambda_reg) over the
// four embedding tables.  nn.Embedding gradients are dense, so every step moves EVERY row (weight decay,
// and the moment/accumulator recurrences of the adaptive optimisers) — reproduced as is:
//
//   mf_mb_grad_kernel   one 16-lane group per rating: prediction, loss, scatter-add of the row gradients
//   mf_mb_apply_kernel  one pass over [U | V | Bu | Bi]: g += wd w, optimiser update, gradient re-zeroed
//
// Update formulas are torch's single-tensor implementations with default hyper-parameters
// (torch/optim/{sgd,adam,rmsprop,adagrad}.py).
//
// Dropout (backend_pt.py:42,59: nn.Dropout(p) on the gathered user rows and on the gathered item rows): the keep masks
// are an input — [n_total][k] bytes each, row b = position b of `order` — drawn by the host exactly as the reference's
// run draws them from torch's CPU generator (cornac_amd/mf.py); a kept factor is scaled by keep_scale = 1 / (1 - p),
// pred = sum_f (u_f m_f)(v_f n_f), and the row gradients carry the same masks (autograd through the two products).

namespace chip {

struct MbTables {
    float *w[4];       // U, V, Bu, Bi
    float *g[4];
    float *s1[4];      // Adam exp_avg | RMSprop square_avg | Adagrad state_sum
    float *s2[4];      // Adam exp_avg_sq
    int64_t end[4];    // exclusive prefix ends of the four segments in the flat index space
};

struct MbOpt {
    int kind;          // CORNAC_HIP_OPT_*
    float lr, wd;
    float beta1, beta2, one_minus_beta1, one_minus_beta2, step_size, bc2_sqrt, eps;  // Adam
    float alpha, one_minus_alpha;                                                    // RMSprop
};

__global__ __launch_bounds__(256) void mf_mb_grad_kernel(const int64_t *__restrict__ order, int64_t n,
                                                         const int64_t *__restrict__ rid,
                                                         const int64_t *__restrict__ cid,
                                                         const float *__restrict__ val, const MbTables t, int k,
                                                         float mu, int use_bias, double *loss,
                                                         const uint8_t *__restrict__ keep_u,
                                                         const uint8_t *__restrict__ keep_i, float keep_scale) {
    __shared__ double scratch[4];
    const int grp = threadIdx.x >> 4, gl = threadIdx.x & 15;
    double part = 0;
    for (int64_t b = (int64_t)blockIdx.x * 16 + grp; b < n; b += (int64_t)gridDim.x * 16) {
        const int64_t e = order[b];
        const int64_t u = rid[e], i = cid[e];
        const float *ur = t.w[0] + u * k, *vr = t.w[1] + i * k;
        const uint8_t *ku = keep_u ? keep_u + b * k : nullptr, *ki = keep_u ? keep_i + b * k : nullptr;
        float p = 0.f;
        if (ku) {
            for (int f = gl; f < k; f += 16) p += (ur[f] * (ku[f] ? keep_scale : 0.f)) * (vr[f] * (ki[f] ? keep_scale : 0.f));
        } else {
            for (int f = gl; f < k; f += 16) p += ur[f] * vr[f];
        }
#pragma unroll
        for (int o = 8; o >= 1; o >>= 1) p += __shfl_xor(p, o, 16);
        if (use_bias) p += t.w[2][u] + t.w[3][i] + mu;
        const float err = p - val[e];
        const float g = 2.f * err;
        if (ku) {
            for (int f = gl; f < k; f += 16) {
                const float mu_f = ku[f] ? keep_scale : 0.f, mi_f = ki[f] ? keep_scale : 0.f;
                atomicAdd(t.g[0] + u * k + f, (g * (vr[f] * mi_f)) * mu_f);
                atomicAdd(t.g[1] + i * k + f, (g * (ur[f] * mu_f)) * mi_f);
            }
        } else
        for (int f = gl; f < k; f += 16) {
            atomicAdd(t.g[0] + u * k + f, g * vr[f]);
            atomicAdd(t.g[1] + i * k + f, g * ur[f]);
        }
        if (gl == 0) {
            if (use_bias) {
                atomicAdd(t.g[2] + u, g);
                atomicAdd(t.g[3] + i, g);
            }
            part += (double)err * err;
        }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) part += __shfl_xor(part, o, 64);
    if ((threadIdx.x & 63) == 0) scratch[threadIdx.x >> 6] = part;
    __syncthreads();
    if (threadIdx.x == 0) {
        const double s = scratch[0] + scratch[1] + scratch[2] + scratch[3];
        if (s != 0) atomicAdd(loss, s);
    }
}

__global__ __launch_bounds__(256) void mf_mb_apply_kernel(const MbTables t, int n_seg, const MbOpt o) {
    const int64_t total = t.end[n_seg - 1];
    for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < total; e += (int64_t)gridDim.x * 256) {
        int s = 0;
        while (e >= t.end[s]) ++s;
        const int64_t off = e - (s ? t.end[s - 1] : 0);
        float w = t.w[s][off];
        float g = t.g[s][off];
        if (g != 0.f) t.g[s][off] = 0.f;
        g = g + o.wd * w;
        if (o.kind == CORNAC_HIP_OPT_SGD) {
            w = w + (-o.lr) * g;
        } else if (o.kind == CORNAC_HIP_OPT_ADAM) {
            float m = t.s1[s][off], v = t.s2[s][off];
            m = m + o.one_minus_beta1 * (g - m);
            v = v * o.beta2;
            v = v + o.one_minus_beta2 * (g * g);
            t.s1[s][off] = m;
            t.s2[s][off] = v;
            const float denom = sqrtf(v) / o.bc2_sqrt + o.eps;
            w = w + (-o.step_size) * (m / denom);
        } else if (o.kind == CORNAC_HIP_OPT_RMSPROP) {
            float sq = t.s1[s][off];
            sq = sq * o.alpha;
            sq = sq + o.one_minus_alpha * (g * g);
            t.s1[s][off] = sq;
            w = w + (-o.lr) * (g / (sqrtf(sq) + o.eps));
        } else {  // Adagrad
            float acc = t.s1[s][off];
            acc = acc + g * g;
            t.s1[s][off] = acc;
            w = w + (-o.lr) * (g / (sqrtf(acc) + o.eps));
        }
        t.w[s][off] = w;
    }
}

}  // namespace chip

extern "C" {

int cornac_hip_mf_reset_optimizer(cornac_hip_mf_t h) {
    return guarded([&] {
        mf_check(h);
        h->opt_step = 0;
        h->opt_kind = -1;
        for (int s = 0; s < 4; ++s) {
            if (h->opt_s1[s].p) HIP_CHECK(hipMemsetAsync(h->opt_s1[s].p, 0, h->opt_s1[s].n * 4, h->stream));
            if (h->opt_s2[s].p) HIP_CHECK(hipMemsetAsync(h->opt_s2[s].p, 0, h->opt_s2[s].n * 4, h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
    });
}

static void mf_fit_minibatch_impl(cornac_hip_mf_t h, const int64_t *order, int64_t n_total, int batch_size, int optimizer,
                                 float lr, float reg, float mu, int use_bias, const uint8_t *keep_u, const uint8_t *keep_i,
                                 float keep_scale, double *loss_sum) {
    {
        mf_check(h);
        REQUIRE(optimizer >= CORNAC_HIP_OPT_SGD && optimizer <= CORNAC_HIP_OPT_ADAGRAD, "unknown optimizer %d", optimizer);
        REQUIRE(batch_size > 0, "batch_size must be positive");
        REQUIRE(n_total >= 0, "n_total < 0");
        REQUIRE(h->opt_kind < 0 || h->opt_kind == optimizer,
                "optimizer changed mid-training; call cornac_hip_mf_reset_optimizer first");
        if (n_total == 0) {
            if (loss_sum) *loss_sum = 0;
            return;
        }
        REQUIRE(order != nullptr, "order is NULL");
        for (int64_t b = 0; b < n_total; ++b)
            REQUIRE(order[b] >= 0 && order[b] < h->nnz, "order[%lld] out of range", (long long)b);
        h->opt_kind = optimizer;
        hipStream_t s = h->stream;
        const int k = h->k;
        const size_t sizes[4] = {(size_t)h->n_users * k, (size_t)h->n_items * k, (size_t)h->n_users, (size_t)h->n_items};
        DevBuf<float> *w[4] = {&h->U, &h->V, &h->Bu, &h->Bi};
        const int n_seg = use_bias ? 4 : 2;  // without biases only the two factor tables are parameters
        MbTables t;
        int64_t end = 0;
        for (int q = 0; q < 4; ++q) {
            if (!h->opt_g[q].p) {
                h->opt_g[q].alloc(sizes[q]);
                HIP_CHECK(hipMemsetAsync(h->opt_g[q].p, 0, sizes[q] * 4, s));
            }
            if (optimizer != CORNAC_HIP_OPT_SGD && !h->opt_s1[q].p) {
                h->opt_s1[q].alloc(sizes[q]);
                HIP_CHECK(hipMemsetAsync(h->opt_s1[q].p, 0, sizes[q] * 4, s));
            }
            if (optimizer == CORNAC_HIP_OPT_ADAM && !h->opt_s2[q].p) {
                h->opt_s2[q].alloc(sizes[q]);
                HIP_CHECK(hipMemsetAsync(h->opt_s2[q].p, 0, sizes[q] * 4, s));
            }
            t.w[q] = w[q]->p; t.g[q] = h->opt_g[q].p; t.s1[q] = h->opt_s1[q].p; t.s2[q] = h->opt_s2[q].p;
            end += (int64_t)sizes[q];
            t.end[q] = end;
        }
        h->opt_order.ensure((size_t)n_total);
        h->opt_order.upload(order, (size_t)n_total, s);
        const uint8_t *d_ku = nullptr, *d_ki = nullptr;
        if (keep_u) {  // the keep masks of this call's batches: [n_total][k] bytes each
            REQUIRE(keep_i != nullptr, "dropout needs both keep masks");
            h->opt_keep.ensure(2 * (size_t)n_total * (size_t)k);
            h->opt_keep.upload(keep_u, (size_t)n_total * (size_t)k, s);
            HIP_CHECK(hipMemcpyAsync(h->opt_keep.p + (size_t)n_total * (size_t)k, keep_i, (size_t)n_total * (size_t)k,
                                     hipMemcpyHostToDevice, s));
            d_ku = h->opt_keep.p;
            d_ki = h->opt_keep.p + (size_t)n_total * (size_t)k;
        }
        h->loss.ensure(1);
        HIP_CHECK(hipMemsetAsync(h->loss.p, 0, sizeof(double), s));
        const int64_t total = t.end[n_seg - 1];
        const int apply_grid = (int)std::max<int64_t>(1, std::min<int64_t>((total + 255) / 256, 8192));
        for (int64_t b0 = 0; b0 < n_total; b0 += batch_size) {
            const int64_t n = std::min<int64_t>(batch_size, n_total - b0);
            ++h->opt_step;
            MbOpt o;
            o.kind = optimizer; o.lr = lr; o.wd = reg;
            // torch holds the betas and alpha as doubles and rounds 1 - beta to float32 when the tensor operation takes it:
            // 1.f - 0.999f is 1.3e-5 below (float)(1.0 - 0.999), which put every early Adam step 6.4e-6 off
            o.beta1 = 0.9f; o.beta2 = 0.999f; o.one_minus_beta1 = (float)(1.0 - 0.9); o.one_minus_beta2 = (float)(1.0 - 0.999);
            const double bc1 = 1.0 - std::pow(0.9, (double)h->opt_step), bc2 = 1.0 - std::pow(0.999, (double)h->opt_step);
            o.step_size = (float)((double)lr / bc1);
            o.bc2_sqrt = (float)std::sqrt(bc2);
            o.eps = optimizer == CORNAC_HIP_OPT_ADAGRAD ? 1e-10f : 1e-8f;
            o.alpha = 0.99f; o.one_minus_alpha = (float)(1.0 - 0.99);
            const int grad_grid = (int)std::max<int64_t>(1, std::min<int64_t>((n + 15) / 16, 4096));
            mf_mb_grad_kernel<<<grad_grid, 256, 0, s>>>(h->opt_order.p + b0, n, h->rid.p, h->cid.p, h->val.p, t, k, mu,
                                                       use_bias, h->loss.p, d_ku ? d_ku + (size_t)b0 * k : nullptr,
                                                       d_ki ? d_ki + (size_t)b0 * k : nullptr, keep_scale);
            mf_mb_apply_kernel<<<apply_grid, 256, 0, s>>>(t, n_seg, o);
        }
        HIP_CHECK(hipGetLastError());
        double l = 0;
        HIP_CHECK(hipMemcpyAsync(&l, h->loss.p, sizeof l, hipMemcpyDeviceToHost, s));
        HIP_CHECK(hipStreamSynchronize(s));
        if (loss_sum) *loss_sum = l;
    }
}

int cornac_hip_mf_fit_minibatch(cornac_hip_mf_t h, const int64_t *order, int64_t n_total, int batch_size,
                                int optimizer, float lr, float reg, float mu, int use_bias, double *loss_sum) {
    return guarded([&] {
        mf_fit_minibatch_impl(h, order, n_total, batch_size, optimizer, lr, reg, mu, use_bias, nullptr, nullptr, 1.f, loss_sum);
    });
}

int cornac_hip_mf_fit_minibatch_dropout(cornac_hip_mf_t h, const int64_t *order, int64_t n_total, int batch_size,
                                        int optimizer, float lr, float reg, float mu, int use_bias, const uint8_t *keep_u,
                                        const uint8_t *keep_i, float keep_scale, double *loss_sum) {
    return guarded([&] {
        REQUIRE(keep_u && keep_i, "keep masks are NULL (cornac_hip_mf_fit_minibatch is the call without dropout)");
        mf_fit_minibatch_impl(h, order, n_total, batch_size, optimizer, lr, reg, mu, use_bias, keep_u, keep_i, keep_scale, loss_sum);
    });
}

}  // extern "C"
