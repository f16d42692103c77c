"""The public-input scheme (include/mfhip.h, mfh_*_public) restated in Python integers on top of tests/test_oracle_python_mirror.py's Mirror: setup with rows
v[0..lu) encrypting 0, the prover with the statement's v_i added into v and left out of w and b_w, the verifier from v_i(s).  Shared by
tests/test_gpu_public_inputs.py (against the GPU bytes) and tests/test_public_inputs_cpu.py (the algebra alone)."""
import oracle_lib as ol

PP = ol.P


def _mirror_public():
    from test_oracle_python_mirror import Mirror

    class PublicMirror(Mirror):
        """the public-input scheme restated on top of Mirror: setup with rows v[0..lu) encrypting 0; prover with w_priv / v split; verifier from the key"""

        def setup_public(self, seed, t, v, alpha, beta, s, sk, errs, lu):
            crs = self.setup(seed, t, v, alpha, beta, s, sk, errs)
            p = self.p
            off = p.ctr_bv
            rows = bytearray(crs["v"])
            for i in range(1, p.m):  # (the stream position of row v[i-1]; only the first lu change)
                if i <= lu:
                    ct, _ = self.encrypt(seed, off, sk, 0, errs[2 * p.d + i])
                    rows[(i - 1) * p.ctb:i * p.ctb] = self.ct_export(ct)
                off += p.n * p.ctb
            crs["v"] = bytes(rows)
            return crs

        def prover_public(self, seed, crs, t, v, bits, lu, delta, smudges):
            p = self.p
            bit = lambda i: (bits[(i - 1) >> 3] >> ((i - 1) & 7)) & 1  # noqa: E731
            w = [c * delta % PP for c in t]
            off = p.ctr_bt
            b_w, off = self.ct_import(seed, off, crs["t"])
            b_w = self.ct_mul_ui(b_w, delta)
            vv = list(v[0])
            for i in range(1, p.m):
                ct, off = self.ct_import(seed, off, crs["v"][(i - 1) * p.ctb:i * p.ctb])
                if bit(i) and i > lu:
                    w = [(x + y) % PP for x, y in zip(w, v[i])]
                    b_w = self.ct_add(b_w, ct)
                elif bit(i):
                    vv = [(x + y) % PP for x, y in zip(vv, v[i])]
            v_w = self.eval_poly(seed, p.ctr_s, crs["s"], w)
            vv = [(x + y) % PP for x, y in zip(vv, w)]
            hat_v = self.eval_poly(seed, p.ctr_as, crs["as_"], vv)
            sq = [0] * (2 * p.d - 1)
            for i, x in enumerate(vv):
                if x:
                    for j, y in enumerate(vv):
                        sq[i + j] = (sq[i + j] + x * y) % PP
            sq[0] = (sq[0] - 1) % PP
            h = self.poly_div(sq, t)
            pi_h = self.eval_poly(seed, p.ctr_s, crs["s"], h)
            hat_h = self.eval_poly(seed, p.ctr_as, crs["as_"], h)
            (m0, s0), (m1, s1), (m2, s2), (m3, s3), (m4, s4) = smudges
            return [self.ct_smudge(pi_h, m0, s0), self.ct_smudge(hat_h, m1, s1), self.ct_smudge(hat_v, m2, s2),
                    self.ct_smudge(self.ct_smudge(v_w, m3, s3), m4, s4), b_w]

        def verifier_public(self, t, v, alpha, beta, s, sk, lu, u, proof):
            h_s, hath_s, hatv_s, w_s, b_s = (self.decrypt(sk, c) for c in proof)
            v_s = (self.poly_eval(v[0], s) + w_s + sum(self.poly_eval(v[i], s) for i in range(1, lu + 1) if (u[(i - 1) >> 3] >> ((i - 1) & 7)) & 1)) % PP
            return (h_s * alpha % PP == hath_s and v_s * alpha % PP == hatv_s and (v_s * v_s - 1 - h_s * self.poly_eval(t, s)) % PP == 0
                    and w_s * beta % PP == b_s)

    return PublicMirror
