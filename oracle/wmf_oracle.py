"""CPU restatement of the reference's WMF training step — TEST INFRASTRUCTURE ONLY.

PARITY: pinned against the reference's OWN WMF code, not against TensorFlow.  The reference computes this path inside
TensorFlow (`tensorflow==2.12.0`, cornac/models/wmf/requirements.txt), which is absent from this image, and no
reference test touches WMF.  What IS checked (tests/test_oracle_vs_reference.py::test_wmf_oracle_and_host_class_match_the_reference_wmf_code,
tests/golden/wmf_ref.npz): cornac/models/wmf/recom_wmf.py + wmf.py run unmodified over oracle/tf1_shim — torch forward
and autograd of the loss THEIR code builds, their xavier initialisation, their item_iter shuffling and batch_C — and
this restatement (hand-derived gradients, loop, Adam) reproduces the result to 5e-6.  What stays restated on both
sides, from TensorFlow's published source rather than by running it: the IndexedSlices gradient of tf.gather,
clip_by_value on it, and tf.train.AdamOptimizer's dense / sparse update rules (listed in the shim's header).

Follows:
  * cornac/models/wmf/wmf.py:34-55        graph: P = U V_b^T, loss = sum(C (R - P)^2) + lambda_u l2(U) + lambda_v l2(V_b)
                                          (tf.nn.l2_loss(x) = sum(x^2) / 2), gradients clipped to [-5, 5]
  * cornac/models/wmf/recom_wmf.py:160-207  one `sess.run(opt)` per batch of items from `item_iter(shuffle=True)`;
                                          C = b everywhere, a where the batch's rating matrix is non-zero
  * TF1 Adam (beta1 .9, beta2 .999, eps 1e-8): lr_t = lr sqrt(1 - beta2^t) / (1 - beta1^t);
    m += (1-beta1)(g - m); v += (1-beta2)(g^2 - v); var -= lr_t m / (sqrt(v) + eps).
    `V` receives an IndexedSlices gradient (tf.gather), for which TF1 Adam decays m, v of ALL rows, adds the
    slice contribution to the gathered rows and then updates ALL rows (`_apply_sparse_shared`).
All arithmetic in float32 like the graph's dtype.

`dtype=np.float64` runs the same step in double precision from the float32 inputs widened (tables and the float32
values of lambda_u, lambda_v, a, b: the device receives floats) — the yardstick of tests/test_wmf_gpu.py.  In that mode
the oracle also keeps, per element of U and V, a first-order bound of what float32 rounding of the GRADIENT can do to
the result:   sens += lr_t (1 - beta1) / (sqrt(v_t) + eps) * 2^-22 * mag,   mag = the sum of the absolute values of the
gradient's terms (|D| |V_b| + lambda_u |U|, resp. |D|^T |U| + lambda_v |V_b|); a step adds nothing where the raw
gradient is clipped (|raw| > 5.001: the clipped value does not depend on it).  Step 1 of Adam moves an element by about
lr sign(g), so an element whose gradient is within rounding of zero is ill-conditioned: `flagged(T)` marks the elements
whose bound exceeds T / 2, and a comparison at T holds for the others.  The bound contains the update rule and float32's
unit roundoff, no fitted constant.  `clip_share` is the share of gradient elements the clip changed, per table.
"""
import numpy as np

f32 = np.float32


class WmfOracle:
    def __init__(self, U, V, csc, lambda_u=0.01, lambda_v=0.01, a=1.0, b=0.01, lr=0.001,
                 beta1=0.9, beta2=0.999, eps=1e-8, dtype=f32):
        ft = self.ft = np.dtype(dtype).type
        self.U = np.array(np.asarray(U, dtype=f32), dtype=ft)
        self.V = np.array(np.asarray(V, dtype=f32), dtype=ft)
        self.R = csc.tocsc()
        self.lu, self.lv, self.a, self.b, self.lr = ft(f32(lambda_u)), ft(f32(lambda_v)), ft(f32(a)), ft(f32(b)), float(lr)
        self.b1, self.b2, self.eps = beta1, beta2, ft(f32(eps))
        self.mU = np.zeros_like(self.U); self.vU = np.zeros_like(self.U)
        self.mV = np.zeros_like(self.V); self.vV = np.zeros_like(self.V)
        self.t = 0
        self.track = ft is np.float64
        if self.track:
            self.sensU = np.zeros_like(self.U); self.sensV = np.zeros_like(self.V)
            self.n_clip = {"U": 0, "V": 0}
            self.n_grad = {"U": 0, "V": 0}

    def flagged(self, T):
        """(mask over U, mask over V) of the elements whose float32 conditioning bound exceeds T / 2"""
        return self.sensU > 0.5 * T, self.sensV > 0.5 * T

    def clip_share(self, table):
        return self.n_clip[table] / max(1, self.n_grad[table])

    def step(self, item_ids):
        ft = self.ft
        ids = np.asarray(item_ids, dtype=np.int64)
        self.t += 1
        b1, b2 = ft(self.b1), ft(self.b2)
        Rb = np.asarray(self.R[:, ids].toarray(), dtype=ft)
        C = np.where(Rb != 0, self.a, self.b).astype(ft)
        Vb = self.V[ids]
        P = self.U @ Vb.T
        E = Rb - P
        loss = float(np.sum(C * E * E, dtype=np.float64) + 0.5 * self.lu * np.sum(self.U.astype(np.float64) ** 2)
                     + 0.5 * self.lv * np.sum(Vb.astype(np.float64) ** 2))
        D = ft(-2.0) * C * E
        rawU, rawV = self.raw_gradients(D, Vb)
        gU = np.clip(rawU, ft(-5), ft(5)).astype(ft)
        gV = np.clip(rawV, ft(-5), ft(5)).astype(ft)
        if self.track:
            aD = np.abs(D)
            magU = aD @ np.abs(Vb) + self.lu * np.abs(self.U)
            magV = aD.T @ np.abs(self.U) + self.lv * np.abs(Vb)
            for n, raw in (("U", rawU), ("V", rawV)):
                self.n_clip[n] += int(np.count_nonzero(np.abs(raw) > 5.0))
                self.n_grad[n] += raw.size
        lr_t = ft(self.lr * np.sqrt(1.0 - self.b2 ** self.t) / (1.0 - self.b1 ** self.t))
        self.mU += (ft(1) - b1) * (gU - self.mU)
        self.vU += (ft(1) - b2) * (gU * gU - self.vU)
        self.U -= lr_t * self.mU / (np.sqrt(self.vU) + self.eps)
        self.mV *= b1
        self.vV *= b2
        self.mV[ids] += (ft(1) - b1) * gV
        self.vV[ids] += (ft(1) - b2) * (gV * gV)
        self.V -= lr_t * self.mV / (np.sqrt(self.vV) + self.eps)
        if self.track:
            w = float(lr_t) * (1.0 - self.b1) * 2.0 ** -22
            self.sensU += w / (np.sqrt(self.vU) + self.eps) * magU * (np.abs(rawU) <= 5.001)
            self.sensV[ids] += w / (np.sqrt(self.vV[ids]) + self.eps) * magV * (np.abs(rawV) <= 5.001)
        return loss

    def raw_gradients(self, D, Vb):
        """(dU, dV) before the clip, D = dLoss/dP  (a method of its own so that a test can plant a defect in one of them)"""
        return D @ Vb + self.lu * self.U, D.T @ self.U + self.lv * Vb

    def fit_batches(self, batches):
        return [self.step(ids) for ids in batches]
