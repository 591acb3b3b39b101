// LightGCN (He et al. 2020; cornac/models/lightgcn/lightgcn.py:13-134, recom_lightgcn.py:143-189) on gfx950, float32
// throughout.  The handle owns the normalised adjacency of the bipartite graph as ONE CSR over the n_users + n_items nodes
// (users first: a user's row lists nu + item, an item's row lists users, i.e. the train matrix and its transpose, with the
// edge weight (deg_u deg_i)^-1/2 in both), the layer-0 tables in one buffer [E0_user | E0_item], Adam's two state buffers of
// the same layout and its step counter.  The graph, the hop, the order, the loss and gradient kernels and Adam's pass are
// graph.h's, shared with ngcf.hip; this file holds LightGCN's epilogue of a hop (the running sum) and its host side.
//
// E = P(E0), P = 1 / (L + 1) sum_{k = 0..L} A^k.  P is linear and symmetric, so dL/dE0 = P(G): the same hops serve both
// directions and nothing of the forward pass is kept but the running sum and two ping-pong buffers.
//
// An epoch's triplets lie on the device before the first step.  Then, with no host synchronisation in between:
//   order      once per epoch, all steps in one launch: each step's users and its items [positives | negatives] sorted by id,
//              stable, by counting (as ncf.hip orders its samples)
//   per step   hop x L     one lane group per node: H'_r = sum_{e in row r} w_e H[src_e], edges ascending, kLgcnAhead source
//                          rows in flight, the edge stream read a group's width at a time and one chunk ahead; S_r += H'_r,
//                          divided by L + 1 at the last layer.  A row longer than kLgcnPiece edges is cut into pieces, one
//                          group each, whose partial sums a second small launch adds in piece order.
//              loss        one wave per triplet: the two scores, softplus, sigmoid, the three squared norms
//              gradient    one thread per entry of G: bisects the step's sorted ids for its node and sums that node's
//                          gradient rows in sample order (float64, rounded once); zero elsewhere
//              hop x L     g = P(G)
//              adam        torch's dense update of every entry of both tables
//   losses     once per epoch: each step's terms summed by a fixed tree in float64
// No atomics; every sum has one fixed order, so the same inputs give the same bits.
#include "graph.h"

namespace chip {
namespace {

// where a hop's result goes: H' (unless this is the last layer), S = Sin + H' (divided by div at the last layer)
struct LgcnOut {
    float *hout;
    const float *sin;
    float *sout;
    int last;
    float div;

    template <int VEC>
    __device__ inline void finish(int64_t row, int c, int d, const LgcnVec<VEC> &h) const {
        const int64_t at = row * d + c;
        if (!last) lgcn_store<VEC>(hout + at, h);
        LgcnVec<VEC> s = lgcn_load<VEC>(sin + at);
#pragma unroll
        for (int q = 0; q < VEC; ++q) {
            s.v[q] = s.v[q] + h.v[q];
            if (last) s.v[q] = s.v[q] / div;
        }
        lgcn_store<VEC>(sout + at, s);
    }
};

}  // namespace
}  // namespace chip

using namespace chip;

struct cornac_hip_lightgcn : ModelHandle {
    LgcnGraphDev g;
    int64_t n_users = 0, n_items = 0, total = 0;   // total: entries of a table pair
    int d = 0, L = 0;
    int64_t t = 0;   // Adam's step counter
    DevBuf<float> w, m, v;          // [E0_user | E0_item] and Adam's state
    std::vector<TableSlot> slots;   // the two tables of w / m / v / E
    DevBuf<float> E, Gr, gs, ha, hb;   // final embeddings, gradient at them, P(gradient), the hops' ping-pong
    LgcnEpoch ep;                   // an epoch's triplets
};

// out = P(in): L hops; in and out are distinct table pairs
static void lgcn_propagate(cornac_hip_lightgcn_t h, const float *in, float *out) {
    if (h->L == 0) {
        HIP_CHECK(hipMemcpyAsync(out, in, (size_t)h->total * sizeof(float), hipMemcpyDeviceToDevice, h->stream));
        return;
    }
    const float *cur = in;
    for (int k = 1; k <= h->L; ++k) {
        float *dst = (k & 1) ? h->ha.p : h->hb.p;
        lgcn_hop(h->g, h->d, cur, LgcnOut{dst, k == 1 ? in : out, out, k == h->L ? 1 : 0, (float)(h->L + 1)}, h->stream);
        cur = dst;
    }
}

int cornac_hip_lightgcn_create(cornac_hip_lightgcn_t *out, int device, int64_t n_users, int64_t n_items, const int64_t *indptr,
                               const int32_t *indices, int emb_size, int num_layers) {
    return guarded([&] {
        REQUIRE(out != nullptr, "out handle pointer is NULL");
        *out = nullptr;
        REQUIRE(n_users > 0 && n_items > 0, "lightgcn: sizes must be positive");
        REQUIRE(n_users + n_items < (1ll << 31), "lightgcn: n_users + n_items must be below 2^31");
        REQUIRE(emb_size >= 1 && emb_size <= kLgcnMaxD, "lightgcn: emb_size = %d is outside the supported range 1 <= emb_size <= %d",
                emb_size, kLgcnMaxD);
        REQUIRE(num_layers >= 0 && num_layers <= kLgcnMaxLayers, "lightgcn: num_layers = %d is outside the supported range 0 <= num_layers <= %d",
                num_layers, kLgcnMaxLayers);
        std::unique_ptr<cornac_hip_lightgcn> h(new cornac_hip_lightgcn());
        const char *nm = "lightgcn";
        h->g.build(nm, n_users, n_items, indptr, indices);
        h->n_users = n_users; h->n_items = n_items;
        h->d = emb_size; h->L = num_layers;
        h->total = h->g.n_nodes * emb_size;
        h->slots = {{0, n_users, emb_size, false}, {n_users * emb_size, n_items, emb_size, false}};
        h->open(device);
        h->g.upload(nm, emb_size, h->stream);
        for (DevBuf<float> *b : {&h->w, &h->m, &h->v, &h->E, &h->Gr, &h->gs, &h->ha, &h->hb}) {
            alloc_named(*b, (size_t)h->total, nm, "the tables, Adam's state and the propagation buffers");
            HIP_CHECK(hipMemsetAsync(b->p, 0, b->n * sizeof(float), h->stream));
        }
        HIP_CHECK(hipStreamSynchronize(h->stream));
        h->g.drop_host();
        *out = h.release();
    });
}

int cornac_hip_lightgcn_destroy(cornac_hip_lightgcn_t h) { return destroy_handle(h); }

static void lgcn_get(cornac_hip_lightgcn_t h, const DevBuf<float> &buf, float *user, float *item) {
    float *const tables[2] = {user, item};
    get_tables(h->stream, buf.p, h->slots, tables);
}

int cornac_hip_lightgcn_set_params(cornac_hip_lightgcn_t h, const float *user, const float *item) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        const float *const tables[2] = {user, item};
        put_tables(h->stream, h->w.p, h->slots, tables);
    });
}

int cornac_hip_lightgcn_get_params(cornac_hip_lightgcn_t h, float *user, float *item) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        lgcn_get(h, h->w, user, item);
    });
}

int cornac_hip_lightgcn_get_state(cornac_hip_lightgcn_t h, float *m_user, float *m_item, float *v_user, float *v_item, int64_t *t) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        lgcn_get(h, h->m, m_user, m_item);
        lgcn_get(h, h->v, v_user, v_item);
        if (t) *t = h->t;
    });
}

int cornac_hip_lightgcn_reset_optimizer(cornac_hip_lightgcn_t h) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        zero_state(h->stream, {&h->m, &h->v});
        h->t = 0;
    });
}

int cornac_hip_lightgcn_propagate(cornac_hip_lightgcn_t h, float *user_out, float *item_out) {
    return guarded([&] {
        check_handle(h, "lightgcn handle");
        lgcn_propagate(h, h->w.p, h->E.p);
        lgcn_get(h, h->E, user_out, item_out);
    });
}

int cornac_hip_lightgcn_fit_epoch(cornac_hip_lightgcn_t h, int64_t steps, const int64_t *step_ptr, const int32_t *users,
                                  const int32_t *pos, const int32_t *neg, float lr, float lambda_reg, double *loss_out,
                                  double *bpr_out, double *reg_out) {
    return guarded([&] {
        // (the steps' shape is checked before the handle: it needs no device)
        const int64_t max_n = LgcnEpoch::check_steps("lightgcn", steps, step_ptr);
        check_handle(h, "lightgcn handle");
        REQUIRE(users && pos && neg, "lightgcn: users / pos / neg are NULL");
        REQUIRE(std::isfinite(lr) && std::isfinite(lambda_reg), "lightgcn: lr and lambda_reg must be finite");
        h->ep.stage("lightgcn", h->n_users, h->n_items, steps, max_n, step_ptr, users, pos, neg, h->stream);
        for (int64_t s = 0; s < steps; ++s) {
            const int64_t base = step_ptr[s], n = step_ptr[s + 1] - base;
            h->t += 1;
            const VaeAdam adam = adam_at(h->t, lr);
            lgcn_propagate(h, h->w.p, h->E.p);
            h->ep.loss_and_gradient(h->E.p, h->d, h->n_users, h->g.n_nodes, base, n, lambda_reg, h->Gr.p, h->stream);
            lgcn_propagate(h, h->Gr.p, h->gs.p);
            lgcn_adam_kernel<<<grid(h->total), kLgcnBlock, 0, h->stream>>>(h->w.p, h->m.p, h->v.p, h->gs.p, h->total, adam);
            HIP_CHECK(hipGetLastError());
        }
        h->ep.losses(steps, (double)lambda_reg, loss_out, bpr_out, reg_out, h->stream);
    });
}
