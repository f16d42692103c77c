// ssp_rows.hip -- the row SSP (mfh_ssp_set_rows): a constraint system kept as its rows, never as the dense (m + 3) x d image.
//
// Points r_j = j + 2, j < n = d - 1, as mfh_ssp_from_rows (ssp_interp.hip).  The prover needs the coefficients of w - delta t = sum_j c_j Q_j,
// c_j = E_j w_j (E_j = the row sum of the statement's selected wires, w_j the Lagrange weight, Q_j = t / (x - r_j)): ONE interpolation per
// statement, computed by the subproduct tree of t.  Leaves (x - r_j), padded with factors x (r = 0, c = 0) to Np = 2^ceil(log2 d) leaves; a node
// of degree L is kept as its L low coefficients (monic).  With N_node = sum_{j in node} c_j T_node / (x - r_j):
//     N_parent = N_L T_R + N_R T_L = N_L T_R' + N_R T_L' + x^L (N_L + N_R)          (T' = T without its leading x^L)
// Bottom: nodes of G = min(64, Np) leaves straight from the rows (k_rows_leaf: the row sums, then the synthetic-division recurrence of k_interp
// in LDS).  Above: every level is one blockwise 3-prime product of length 2L over the whole padded vector (ntt.hpp): forward transforms of
// [N_L, 0] and [N_R, 0], a pointwise product with the cached transforms of [T_R', 0] and [T_L', 0], an inverse transform, CRT and the x^L term.
// A coefficient of the two products is < 2 L p^2 <= 2^86 < p1 p2 p3 (Np <= 2^22), so the CRT is exact and every level is canonical in [0, p).
// The root is x^(Np - n) (w - delta t): shifted down, delta t added.  The interpolant of degree < d - 1 is unique, so the result equals the
// dense SSP's sum_i a_i v_i + delta t bit for bit.
//
// Per context (d alone): the tree of t (bottom nodes, the transforms of every upper level), t itself and the weights.  Per registration: the
// rows (device, row-major; host copy for setup) and the dense prefix of slots [0, lu_max + 2) -- t, v_0, v_1 .. v_lu_max -- which is all that
// k_add_slot / k_add_public / k_eval_slots01 ever read.  Setup evaluates v_i(s) = sum_j V_ij lambda_j(s), lambda_j(s) = w_j t(s) / (s - r_j)
// (the indicator [j = k] at s = r_k) on the host: O(nnz + d) once per setup.
//
// The row check (mfh_ssp_rows_violations, k_rows_violations): the same row sums E_j, wire 0 included, compared with +-1 per statement -- the number of
// violated rows and the first of them, without the tree.
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "ntt.hpp"

using namespace mf_ntt;

namespace {

constexpr uint32_t kLeafMax = 64;               // leaves per bottom node
constexpr size_t kChunkBytes = (size_t)128 << 20;  // interpolation scratch per chunk of statements: 8 words per padded point and statement
constexpr size_t kViolStageBytes = (size_t)64 << 20;  // mfh_ssp_rows_violations: staged witness bits per chunk of statements (at least one statement)

// the bottom nodes of the tree of t: node k = prod_{l < G} (x - r_{kG + l}) (r = 0 past n), its G low coefficients.  One thread per node.
__global__ __launch_bounds__(64) void k_rows_tree_bottom(uint32_t n, uint32_t G, uint32_t nodes, uint32_t *__restrict__ tb) {
  __shared__ uint32_t sm[kLeafMax + 1][64];
  const uint32_t node = blockIdx.x * 64 + threadIdx.x;
  if (node >= nodes) return;
  uint32_t *cf = &sm[0][threadIdx.x];  // coefficient k at cf[64 k]
  cf[0] = 1;
  for (uint32_t l = 0; l < G; l++) {  // multiply by (x - r): c_k <- c_{k-1} - r c_k, degree l -> l + 1
    const uint32_t j = node * G + l, nr = j < n ? P32 - (j + 2) : 0u;
    cf[64 * (l + 1)] = cf[64 * l];
    for (uint32_t k = l; k > 0; k--) cf[64 * k] = red_p32((uint64_t)nr * cf[64 * k] + cf[64 * (k - 1)]);
    cf[0] = mulp(nr, cf[0]);
  }
  for (uint32_t k = 0; k < G; k++) tb[(size_t)node * G + k] = cf[64 * k];
}

// Bottom nodes of the interpolation for `gridDim.y` statements: lane l of node blockIdx.x is leaf j = node G + l.  Its value c_j = E_j w_j, with
// E_j = sum of the row's coefficients over the selected wires: bits != nullptr -- wires i >= 1 whose bit i - 1 of the statement is set (bits + s * stride);
// else column col0 + s (wire 0 also 1 on the padding rows j >= nrows).  Then c_j q_{j,k} for k = G - 1 .. 0 (q_{G-1} = 1, q_{k-1} = T_k + r_j q_k: T_node / (x - r_j))
// into LDS, and lane k sums its coefficient over the leaves.
__global__ __launch_bounds__(64) void k_rows_leaf(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ wire, const uint32_t *__restrict__ coef,
                                                  uint32_t nrows, uint32_t n, const uint8_t *__restrict__ bits, uint32_t stride, uint32_t col0,
                                                  const uint32_t *__restrict__ wj, const uint32_t *__restrict__ tb, uint32_t G, uint32_t Np,
                                                  uint32_t *__restrict__ out) {
  __shared__ uint32_t sm[kLeafMax][kLeafMax + 1];
  const uint32_t l = threadIdx.x, node = blockIdx.x, s = blockIdx.y;
  const uint32_t j = node * G + l;
  if (l < G) {
    uint64_t acc = 0;
    if (j < nrows) {
      const uint8_t *b = bits ? bits + (size_t)s * stride : nullptr;
      const uint32_t col = col0 + s;
      for (uint32_t e = row_ptr[j], e1 = row_ptr[j + 1]; e < e1; e++) {
        const uint32_t wi = wire[e];
        const bool sel = b ? wi >= 1 && ((b[(wi - 1) >> 3] >> ((wi - 1) & 7)) & 1) : wi == col;
        if (sel) acc += coef[e];
      }
    } else if (j < n && !bits && col0 + s == 0) {
      acc = 1;  // padding row: v_0(r_j) = 1
    }
    const uint32_t c = j < n ? mulp(red_p32(acc), wj[j]) : 0u;
    const uint64_t r = j < n ? j + 2 : 0;
    const uint32_t *T = tb + (size_t)node * G;
    uint32_t q = 1;
    for (uint32_t k = G; k-- > 0;) {
      sm[k][l] = mulp(c, q);
      if (k) q = red_p32(r * q + T[k]);
    }
  }
  __syncthreads();
  if (l < G) {
    uint64_t acc = 0;
    for (uint32_t u = 0; u < G; u++) acc += sm[l][u];
    out[(size_t)s * Np + (size_t)node * G + l] = red_p32(acc);
  }
}

// level L -> the operands of the products of length 2L: A block k = [N_{2k}, 0], B block k = [N_{2k+1}, 0] as Montgomery residues of the three primes.
// nv: [ns][Np] coefficients; ab: A = [ns][3][Np], B at ab + b_gap.
__global__ void k_rows_level_load(const uint32_t *__restrict__ nv, uint32_t L, uint32_t Np, Primes3 P, uint32_t *__restrict__ ab, size_t b_gap) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (i >= Np) return;
  const bool low = (i & (2 * L - 1)) < L;
  const uint32_t a = low ? nv[(size_t)s * Np + i] : 0u, b = low ? nv[(size_t)s * Np + i + L] : 0u;
#pragma unroll
  for (int q = 0; q < 3; q++) {
    const NttPrime pq = P.q[q];
    const size_t o = ((size_t)s * 3 + q) * Np + i;
    ab[o] = mont_mul(a, pq.r2, pq.p, pq.ninv);
    ab[b_gap + o] = mont_mul(b, pq.r2, pq.p, pq.ninv);
  }
}
// pointwise, grid.y = 3 * statements: hl == nullptr (the tree of t): C = A B; else C = A hr + B hl with the level's cached transforms of [T_R', 0] / [T_L', 0]
__global__ void k_rows_level_mul(const uint32_t *ab, size_t b_gap, const uint32_t *__restrict__ hl, const uint32_t *__restrict__ hr, uint32_t Np, Primes3 P,
                                 uint32_t *cout) {  // (cout may be ab: each thread reads its A word before it writes it)
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= Np) return;
  const uint32_t q = blockIdx.y % 3;
  const NttPrime pq = P.q[q];
  const size_t o = (size_t)blockIdx.y * Np + i, h = (size_t)q * Np + i;
  const uint32_t a = ab[o], b = ab[b_gap + o];
  cout[o] = hl ? add_mod(mont_mul(a, hr[h], pq.p, pq.ninv), mont_mul(b, hl[h], pq.p, pq.ninv), pq.p) : mont_mul(a, b, pq.p, pq.ninv);
}
// the products back to F_p (CRT) plus x^L (N_L + N_R): level 2L
__global__ void k_rows_level_crt(const uint32_t *__restrict__ cres, const uint32_t *__restrict__ nv, uint32_t L, uint32_t Np, Primes3 P, Crt C,
                                 uint32_t *__restrict__ nout) {
  const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (i >= Np) return;
  const uint32_t *r = cres + (size_t)s * 3 * Np;
  uint64_t x = crt_coeff(r[i], r[(size_t)Np + i], r[(size_t)2 * Np + i], P, C);
  if ((i & (2 * L - 1)) >= L) x += (uint64_t)nv[(size_t)s * Np + i - L] + nv[(size_t)s * Np + i];
  nout[(size_t)s * Np + i] = red_p32(x);
}
// the root: out[k] = root[k + Np - n] (k < n) + delta t_k; t_mode: the root IS x^(Np - n) t, out = t (t_n = 1)
__global__ void k_rows_root(const uint32_t *__restrict__ root, uint32_t Np, uint32_t n, const uint32_t *__restrict__ t, const uint32_t *__restrict__ delta,
                            int t_mode, uint32_t *__restrict__ out, size_t out_stride) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x, s = blockIdx.y;
  if (k > n) return;
  const uint32_t x = k < n ? root[(size_t)s * Np + k + Np - n] : (t_mode ? 1u : 0u);
  out[(size_t)s * out_stride + k] = delta ? red_p32((uint64_t)x + mulp(delta[s], t[k])) : x;
}

// The row check (mfh_ssp_rows_violations): thread (j, s) forms E_j of statement s = blockIdx.y as k_rows_leaf does, from the packed bits, but WITH the
// wire-0 entries (k_rows_leaf leaves them to delta t), and row j is violated unless E_j is 1 or p - 1.  Each wave ballots its violations; the lowest
// violating lane adds their number to count[s] and lowers first[s] to its own row (the lowest of the wave).  Add and min commute: the result does not
// depend on the order the waves arrive in.  A wave without a violation issues no atomic.
__global__ __launch_bounds__(256) void k_rows_violations(const uint32_t *__restrict__ row_ptr, const uint32_t *__restrict__ wire, const uint32_t *__restrict__ coef,
                                                         uint32_t nrows, const uint8_t *__restrict__ bits, uint32_t stride, uint32_t *__restrict__ count,
                                                         uint32_t *__restrict__ first) {
  const uint32_t j = blockIdx.x * 256 + threadIdx.x, s = blockIdx.y;
  bool bad = false;
  if (j < nrows) {
    const uint8_t *b = bits + (size_t)s * stride;
    uint64_t acc = 0;  // each term < 2^32: 2^32 terms fit
    for (uint32_t e = row_ptr[j], e1 = row_ptr[j + 1]; e < e1; e++) {
      const uint32_t wi = wire[e];
      if (wi == 0 || ((b[(wi - 1) >> 3] >> ((wi - 1) & 7)) & 1)) acc += coef[e];
    }
    const uint32_t E = red_p32(acc);
    bad = E != 1 && E != P32 - 1;
  }
  const unsigned long long mask = __ballot(bad);  // 64 lanes; the lanes past nrows vote 0
  if (mask && (threadIdx.x & 63) == (uint32_t)__ffsll(mask) - 1) {
    atomicAdd(count + s, (uint32_t)__popcll(mask));
    atomicMin(first + s, j);
  }
}

inline dim3 g1(uint32_t n, uint32_t y = 1) { return dim3((n + 255) / 256, y); }

}  // namespace

// per context: the tree of t (d alone)
struct RowsTree {
  uint32_t d = 0, n = 0, Np = 0, logNp = 0, G = 0, logG = 0, nlev = 0;
  uint32_t *tb = nullptr;    // bottom nodes, Np words
  uint32_t *hats = nullptr;  // level lev (L = G 2^lev): [2][3][Np] transforms of [T_L', 0] | [T_R', 0]
  uint32_t *d_t = nullptr;   // t, d words zero-padded to a multiple of 32 (the sub-tiles of k_interp and k_seed_local, ssp_interp.hip)
  uint32_t *d_w = nullptr;   // Lagrange weights, n words
  std::vector<uint32_t> h_t, h_w;
  ~RowsTree() {
    for (uint32_t *p : {tb, hats, d_t, d_w})
      if (p) hipFree(p);
  }
};
// per registration
struct SspRows {
  uint32_t nrows = 0, lu_max = 0;
  uint32_t *d_rows = nullptr;  // row_ptr (nrows + 1, from 0) | wire (nnz) | coef (nnz)
  uint32_t *d_prefix = nullptr;  // slots [0, lu_max + 2) in the dense layout
  std::vector<uint32_t> h_ptr, h_wire, h_coef;
  DevBuf ws;  // interpolation scratch
  ~SspRows() {
    if (d_rows) hipFree(d_rows);
    if (d_prefix) hipFree(d_prefix);
    dev_free(ws);
  }
  const uint32_t *row_ptr() const { return d_rows; }
  const uint32_t *wire() const { return d_rows + nrows + 1; }
  const uint32_t *coef() const { return d_rows + nrows + 1 + h_wire.size(); }
};

void ssp_rows_free(mfh_ctx *c, bool tree) {
  if (!c->rows && !(tree && c->rows_tree)) return;
  if (c->stream) hipStreamSynchronize(c->stream);
  if (c->side) hipStreamSynchronize(c->side);
  delete c->rows;
  c->rows = nullptr;
  if (tree) {
    delete c->rows_tree;
    c->rows_tree = nullptr;
  }
  c->rows_prefix = nullptr;
  c->rows_lu_max = 0;
}

namespace {

// one upper level of either tree: nv (level L, ns vectors of Np) -> nout (level 2L).  ab: [2][ns][3][Np] operands; hats of this level: nullptr for the
// tree of t (its operands ARE the level's transforms: ab points into T->hats), else the cached ones.
void rows_level(mfh_ctx *c, const RowsTree *T, uint32_t lev, uint32_t ns, const uint32_t *nv, uint32_t *ab, const uint32_t *hats, uint32_t *cres,
                uint32_t *nout) {
  const uint32_t Np = T->Np, L = T->G << lev, logB = T->logG + lev + 1;
  const size_t gap = (size_t)ns * 3 * Np;
  const Primes3 &P = ntt_primes(c);
  hipLaunchKernelGGL(k_rows_level_load, g1(Np, ns), dim3(256), 0, c->stream, nv, L, Np, P, ab, gap);
  ntt_blocks_forward(c, ab, Np, logB, 2 * ns);
  hipLaunchKernelGGL(k_rows_level_mul, g1(Np, 3 * ns), dim3(256), 0, c->stream, (const uint32_t *)ab, gap, hats, hats ? hats + (size_t)3 * Np : nullptr, Np, P,
                     cres);
  ntt_blocks_inverse(c, cres, Np, logB, ns);
  hipLaunchKernelGGL(k_rows_level_crt, g1(Np, ns), dim3(256), 0, c->stream, (const uint32_t *)cres, nv, L, Np, P, ntt_crt_make(c, logB), nout);
}

int rows_tree_build(mfh_ctx *c, const char *who) {
  const uint32_t d = c->P.d;
  if (c->rows_tree && c->rows_tree->d == d) return MFH_OK;
  if (d > (1u << 22)) { c->err = std::string(who) + ": d above 2^22 exceeds the CRT bound of the tree"; return MFH_EUNSUPPORTED; }
  RowsTree *T = new RowsTree();
  struct Guard { RowsTree *&p; ~Guard() { delete p; } } guard{T};
  T->d = d;
  T->n = d - 1;
  T->Np = 1;
  while (T->Np < d) { T->Np <<= 1; T->logNp++; }
  T->G = std::min(kLeafMax, T->Np);
  while ((1u << T->logG) < T->G) T->logG++;
  T->nlev = T->logNp - T->logG;
  const uint32_t Np = T->Np, n = T->n, Dp = (d + 31) & ~31u;
  if (T->nlev) {
    if (int rc = ntt_reserve(c, T->logNp)) return rc;
  }
  uint32_t *scr = nullptr;  // one operand pair's products and two level vectors
  if (hipMalloc(&T->tb, (size_t)Np * 4) != hipSuccess || hipMalloc(&T->d_t, (size_t)Dp * 4) != hipSuccess || hipMalloc(&T->d_w, (size_t)n * 4) != hipSuccess ||
      (T->nlev && hipMalloc(&T->hats, (size_t)T->nlev * 6 * Np * 4) != hipSuccess) || hipMalloc(&scr, (size_t)5 * Np * 4) != hipSuccess) {
    (void)hipGetLastError();
    if (scr) hipFree(scr);
    c->err = std::string(who) + ": no memory for the tree of t";
    return MFH_ENOMEM;
  }
  struct Free { uint32_t *p; ~Free() { hipFree(p); } } fscr{scr};
  uint32_t *cres = scr, *lv[2] = {scr + (size_t)3 * Np, scr + (size_t)4 * Np};
  const uint32_t nodes = Np / T->G;
  hipLaunchKernelGGL(k_rows_tree_bottom, dim3((nodes + 63) / 64), dim3(64), 0, c->stream, n, T->G, nodes, T->tb);
  HIP_TRY(c, hipMemcpyAsync(lv[0], T->tb, (size_t)Np * 4, hipMemcpyDeviceToDevice, c->stream));
  int cur = 0;
  for (uint32_t lev = 0; lev < T->nlev; lev++) {
    rows_level(c, T, lev, 1, lv[cur], T->hats + (size_t)lev * 6 * Np, nullptr, cres, lv[cur ^ 1]);
    cur ^= 1;
  }
  HIP_TRY(c, hipMemsetAsync(T->d_t, 0, (size_t)Dp * 4, c->stream));  // (the words past d stay zero)
  hipLaunchKernelGGL(k_rows_root, g1(d), dim3(256), 0, c->stream, (const uint32_t *)lv[cur], Np, n, (const uint32_t *)nullptr, (const uint32_t *)nullptr, 1, T->d_t,
                     (size_t)0);
  T->h_t.resize(d);
  HIP_TRY(c, hipMemcpyAsync(T->h_t.data(), T->d_t, (size_t)d * 4, hipMemcpyDeviceToHost, c->stream));
  // w_j = 1 / ((-1)^(n-1-j) j! (n-1-j)!)
  std::vector<uint32_t> invf(n);
  uint32_t f = 1;
  for (uint32_t i = 1; i < n; i++) f = mulp(f, i);
  invf[n - 1] = invp(f);
  for (uint32_t i = n - 1; i > 0; i--) invf[i - 1] = mulp(invf[i], i);
  T->h_w.resize(n);
  for (uint32_t j = 0; j < n; j++) {
    const uint32_t x = mulp(invf[j], invf[n - 1 - j]);
    T->h_w[j] = ((n - 1 - j) & 1) && x ? P32 - x : x;
  }
  HIP_TRY(c, hipMemcpyAsync(T->d_w, T->h_w.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { c->err = std::string(who) + ": building the tree of t failed"; return MFH_EDEVICE; }
  delete c->rows_tree;
  c->rows_tree = T;
  T = nullptr;
  return MFH_OK;
}

// ns interpolations on c->stream: statement s selects by its bits (d_bits + s * stride) or, d_bits == nullptr, column col0 + s; out + s * out_stride
// gets d coefficients, plus d_delta[s] t when d_delta != nullptr.  Scratch: 8 Np words per statement in flight, chunks of at most kChunkBytes.
int rows_interp(mfh_ctx *c, SspRows *R, uint32_t ns, const uint8_t *d_bits, uint32_t stride, uint32_t col0, const uint32_t *d_delta, uint32_t *out,
                size_t out_stride) {
  const RowsTree *T = c->rows_tree;
  const uint32_t Np = T->Np, n = T->n;
  const size_t per = (size_t)8 * Np * 4;
  // (the transforms launch grid.y = 6 ch: at most 65535)
  const uint32_t ch = (uint32_t)std::min<size_t>({(size_t)ns, std::max<size_t>(1, kChunkBytes / per), (size_t)(65535 / 6)});
  if (int rc = work_reserve(c, R->ws, ch * per)) return rc;
  uint32_t *ab = R->ws.as<uint32_t>(), *cres = ab, *lv[2] = {ab + (size_t)6 * ch * Np, ab + (size_t)7 * ch * Np};
  // (cres reuses the A operands: k_rows_level_mul reads A and B at the same index and writes C there)
  for (uint32_t s0 = 0; s0 < ns; s0 += ch) {
    const uint32_t k = std::min(ch, ns - s0);
    hipLaunchKernelGGL(k_rows_leaf, dim3(Np / T->G, k), dim3(64), 0, c->stream, R->row_ptr(), R->wire(), R->coef(), R->nrows, n,
                       d_bits ? d_bits + (size_t)s0 * stride : nullptr, stride, col0 + s0, (const uint32_t *)T->d_w, (const uint32_t *)T->tb, T->G, Np, lv[0]);
    int cur = 0;
    for (uint32_t lev = 0; lev < T->nlev; lev++) {
      rows_level(c, T, lev, k, lv[cur], ab, T->hats + (size_t)lev * 6 * Np, cres, lv[cur ^ 1]);
      cur ^= 1;
    }
    hipLaunchKernelGGL(k_rows_root, g1(n + 1, k), dim3(256), 0, c->stream, (const uint32_t *)lv[cur], Np, n, (const uint32_t *)T->d_t,
                       d_delta ? d_delta + s0 : nullptr, 0, out + (size_t)s0 * out_stride, out_stride);
  }
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

}  // namespace

int ssp_rows_check(mfh_ctx *c, const char *who, uint32_t nrows, const uint32_t *h_row_ptr, const uint32_t *h_wire, const uint32_t *h_coef) {
  const uint32_t d = c->P.d, m = c->P.m;
  auto fail = [&](const char *what) {
    c->err = std::string(who) + ": " + what;
    return MFH_EINVAL;
  };
  if (d < 2) return fail("d < 2");
  if (nrows > d - 1) return fail("nrows > d - 1");
  for (uint32_t j = 0; j < nrows; j++)
    if (h_row_ptr[j + 1] < h_row_ptr[j]) return fail("row_ptr decreases");
  const uint32_t e0 = h_row_ptr[0], e1 = h_row_ptr[nrows];
  if (e1 > e0 && (!h_wire || !h_coef)) return fail("entries without h_wire / h_coef");
  for (uint32_t e = e0; e < e1; e++) {
    if (h_wire[e] >= m) return fail("wire >= m");
    if (h_coef[e] >= P32) return fail("coefficient >= p");
  }
  return MFH_OK;
}

int ssp_rows_tree(mfh_ctx *c, const char *who, const uint32_t *&d_t, const uint32_t *&h_w) {
  if (int rc = rows_tree_build(c, who)) return rc;
  d_t = c->rows_tree->d_t;
  h_w = c->rows_tree->h_w.data();
  return MFH_OK;
}

// the witness polynomials of nstmt statements in row mode (mfh_witness_poly*, the batch chain): d_w + b * w_stride = delta_b t + sum_{bit} v_i
int ssp_rows_witness(mfh_ctx *c, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, const uint32_t *h_delta, uint32_t *d_w, size_t w_stride) {
  SspRows *R = c->rows;
  if (!R || !c->rows_tree) { c->err = "no row SSP registered"; return MFH_EINVAL; }
  if (!nstmt) return MFH_OK;
  for (uint32_t b = 0; b < nstmt; b++)
    if (h_delta[b] >= P32) { c->err = "delta must be < p"; return MFH_EINVAL; }
  const uint32_t bs = (c->P.m + 6) / 8;
  if (bits_stride < bs) { c->err = "bits_stride shorter than the m - 1 witness bits"; return MFH_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  // staged: deltas | bits, compacted to bs bytes per statement; on the device in the tail of the witness scratch
  const size_t db = ((size_t)nstmt * 4 + 255) & ~(size_t)255, bb = (size_t)nstmt * bs;
  uint8_t *st = (uint8_t *)pin_acquire(c, c->pin_rows, db + bb);
  if (!st) return MFH_ENOMEM;
  memcpy(st, h_delta, (size_t)nstmt * 4);
  for (uint32_t b = 0; b < nstmt; b++) memcpy(st + db + (size_t)b * bs, h_bits + (size_t)b * bits_stride, bs);
  if (int rc = wws_reserve(c, db + bb)) return rc;
  HIP_TRY(c, hipMemcpyAsync(c->wws.p, st, db + bb, hipMemcpyHostToDevice, c->stream));
  pin_release(c, c->pin_rows);
  return rows_interp(c, R, nstmt, c->wws.as<const uint8_t>() + db, bs, 0, c->wws.as<const uint32_t>(), d_w, w_stride);
}

// setup messages 2d .. 2d + m - 1 in row mode: beta t(s), beta v_r(s) for r = 1 .. m - 1, from lambda_j(s) (host, O(nnz + d))
int ssp_rows_msg_evals(mfh_ctx *c, uint32_t s, uint32_t beta, uint32_t *d_msg_evals) {
  const SspRows *R = c->rows;
  const RowsTree *T = c->rows_tree;
  const uint32_t d = c->P.d, m = c->P.m, n = d - 1;
  std::vector<uint32_t> lam(n, 0);
  uint32_t ts = 0;
  for (uint32_t k = d; k-- > 0;) ts = (uint32_t)(((uint64_t)ts * s + T->h_t[k]) % P32);
  if (s >= 2 && s - 2 < n) {
    lam[s - 2] = 1;  // s = r_k: lambda_j = [j = k] (t(s) = 0)
  } else {
    // batch inversion of s - r_j
    std::vector<uint32_t> pre(n);
    uint32_t acc = 1;
    for (uint32_t j = 0; j < n; j++) {
      pre[j] = acc;
      acc = mulp(acc, (uint32_t)(((uint64_t)s + P32 - (j + 2)) % P32));
    }
    uint32_t inv = invp(acc);
    for (uint32_t j = n; j-- > 0;) {
      const uint32_t x = (uint32_t)(((uint64_t)s + P32 - (j + 2)) % P32);
      lam[j] = mulp(mulp(inv, pre[j]), mulp(T->h_w[j], ts));
      inv = mulp(inv, x);
    }
  }
  std::vector<uint64_t> acc(m, 0);  // each term < 2^32: 2^32 terms fit
  for (uint32_t j = 0; j < R->nrows; j++)
    for (uint32_t e = R->h_ptr[j]; e < R->h_ptr[j + 1]; e++) acc[R->h_wire[e]] += mulp(R->h_coef[e], lam[j]);
  std::vector<uint32_t> msg(m);
  msg[0] = mulp(ts, beta);
  for (uint32_t r = 1; r < m; r++) msg[r] = mulp((uint32_t)(acc[r] % P32), beta);
  HIP_TRY(c, hipMemcpyAsync(d_msg_evals, msg.data(), (size_t)m * 4, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));  // (msg is on this stack)
  return MFH_OK;
}

extern "C" {

int mfh_ssp_set_rows(mfh_ctx *c, uint32_t nrows, const uint32_t *h_row_ptr, const uint32_t *h_wire, const uint32_t *h_coef, uint32_t lu_max) {
  if (!c) return MFH_EINVAL;
  if (!h_row_ptr) {
    if (nrows) return MFH_EINVAL;
    HIP_TRY(c, hipSetDevice(c->device));
    ssp_rows_free(c, true);  // unregister: the registration and the tree of t
    return MFH_OK;
  }
  // before anything changes
  if (int rc = ssp_rows_check(c, "mfh_ssp_set_rows", nrows, h_row_ptr, h_wire, h_coef)) return rc;
  const uint32_t d = c->P.d, e0 = h_row_ptr[0], e1 = h_row_ptr[nrows];
  if (lu_max >= c->P.m) { c->err = "mfh_ssp_set_rows: lu_max must be < m"; return MFH_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  if (int rc = rows_tree_build(c, "mfh_ssp_set_rows")) return rc;
  SspRows *R = new SspRows();
  struct Guard { SspRows *p; ~Guard() { delete p; } } guard{R};
  R->nrows = nrows;
  R->lu_max = lu_max;
  R->h_ptr.resize(nrows + 1);
  for (uint32_t j = 0; j <= nrows; j++) R->h_ptr[j] = h_row_ptr[j] - e0;
  R->h_wire.assign(h_wire + e0, h_wire + e1);  // (e1 == e0: empty, h_wire may be NULL -- then the range is empty too)
  R->h_coef.assign(h_coef + e0, h_coef + e1);
  const size_t nnz = e1 - e0, rows_w = nrows + 1 + 2 * nnz;
  if (hipMalloc(&R->d_rows, rows_w * 4) != hipSuccess || hipMalloc(&R->d_prefix, (size_t)(lu_max + 2) * d * 4) != hipSuccess) {
    (void)hipGetLastError();
    c->err = "mfh_ssp_set_rows: no memory for the rows";
    return MFH_ENOMEM;
  }
  HIP_TRY(c, hipMemcpyAsync(R->d_rows, R->h_ptr.data(), (size_t)(nrows + 1) * 4, hipMemcpyHostToDevice, c->stream));
  if (nnz) {
    HIP_TRY(c, hipMemcpyAsync(R->d_rows + nrows + 1, R->h_wire.data(), nnz * 4, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(c, hipMemcpyAsync(R->d_rows + nrows + 1 + nnz, R->h_coef.data(), nnz * 4, hipMemcpyHostToDevice, c->stream));
  }
  HIP_TRY(c, hipMemcpyAsync(R->d_prefix, c->rows_tree->d_t, (size_t)d * 4, hipMemcpyDeviceToDevice, c->stream));
  if (int rc = rows_interp(c, R, lu_max + 1, nullptr, 0, 0, nullptr, R->d_prefix + d, d)) return rc;  // v_0 .. v_lu_max
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "mfh_ssp_set_rows: interpolation failed"; return MFH_EDEVICE; }
  // swap: the previous registration (row or generator-defined) is replaced; derived images of the SSP are stale
  if (c->side) hipStreamSynchronize(c->side);
  delete c->rows;
  c->rows = R;
  guard.p = nullptr;
  c->rows_prefix = R->d_prefix;
  c->rows_lu_max = lu_max;
  c->prg_on = false;
  c->prg_t = nullptr;
  ssp_images_stale(c);
  return MFH_OK;
}

int mfh_ssp_rows_fill(mfh_ctx *c, size_t first_slot, size_t nslots, uint32_t *d_out) {
  if (!c || (nslots && !d_out)) return MFH_EINVAL;
  if (!c->rows) { c->err = "mfh_ssp_rows_fill: no row SSP registered (mfh_ssp_set_rows)"; return MFH_EINVAL; }
  const uint32_t d = c->P.d, m = c->P.m;
  if (first_slot + nslots > (size_t)m + 3) { c->err = "mfh_ssp_rows_fill: slots beyond m + 2"; return MFH_EINVAL; }
  HIP_TRY(c, hipSetDevice(c->device));
  for (size_t k = 0; k < nslots;) {
    const size_t slot = first_slot + k;
    uint32_t *o = d_out + k * d;
    if (slot == 0) {
      HIP_TRY(c, hipMemcpyAsync(o, c->rows_tree->d_t, (size_t)d * 4, hipMemcpyDeviceToDevice, c->stream));
      k++;
    } else if (slot > m) {
      HIP_TRY(c, hipMemsetAsync(o, 0, (size_t)d * 4, c->stream));
      k++;
    } else {  // wires slot - 1 .. : columns
      const uint32_t cnt = (uint32_t)std::min<size_t>(nslots - k, (size_t)m + 1 - slot);
      if (int rc = rows_interp(c, c->rows, cnt, nullptr, 0, (uint32_t)slot - 1, nullptr, o, d)) return rc;
      k += cnt;
    }
  }
  HIP_TRY(c, hipGetLastError());
  return MFH_OK;
}

int mfh_ssp_rows_violations(mfh_ctx *c, uint32_t nstmt, const uint8_t *h_bits, size_t bits_stride, uint32_t *h_count, uint32_t *h_first) {
  if (!c) return MFH_EINVAL;
  const SspRows *R = c->rows;
  if (!R) { c->err = "mfh_ssp_rows_violations: no row SSP registered (mfh_ssp_set_rows)"; return MFH_EINVAL; }
  const uint32_t bs = (c->P.m + 6) / 8;
  if (bits_stride < bs) { c->err = "mfh_ssp_rows_violations: bits_stride shorter than the m - 1 witness bits"; return MFH_EINVAL; }
  if (nstmt && (!h_bits || !h_count)) { c->err = "mfh_ssp_rows_violations: statements without h_bits / h_count"; return MFH_EINVAL; }
  if (!nstmt) return MFH_OK;
  HIP_TRY(c, hipSetDevice(c->device));
  // staged as ssp_rows_witness stages them: compacted to bs bytes per statement in pin_rows (mfh_scrub_staging covers it), on the device in the witness
  // scratch: bits | count | first of one chunk of statements
  const uint32_t ch = (uint32_t)std::min<size_t>({(size_t)nstmt, std::max<size_t>(1, kViolStageBytes / bs), (size_t)65535});  // (grid.y <= 65535)
  const size_t bb = ((size_t)ch * bs + 255) & ~(size_t)255;
  if (int rc = wws_reserve(c, bb + (size_t)ch * 8)) return rc;
  const uint8_t *d_bits = c->wws.as<const uint8_t>();
  uint32_t *d_count = reinterpret_cast<uint32_t *>(c->wws.as<uint8_t>() + bb), *d_first = d_count + ch;
  for (uint32_t s0 = 0; s0 < nstmt; s0 += ch) {
    const uint32_t k = std::min(ch, nstmt - s0);
    uint8_t *st = (uint8_t *)pin_acquire(c, c->pin_rows, (size_t)k * bs);
    if (!st) return MFH_ENOMEM;
    for (uint32_t b = 0; b < k; b++) memcpy(st + (size_t)b * bs, h_bits + (size_t)(s0 + b) * bits_stride, bs);
    HIP_TRY(c, hipMemcpyAsync(c->wws.p, st, (size_t)k * bs, hipMemcpyHostToDevice, c->stream));
    pin_release(c, c->pin_rows);
    HIP_TRY(c, hipMemsetAsync(d_count, 0, (size_t)k * 4, c->stream));
    HIP_TRY(c, hipMemsetAsync(d_first, 0xFF, (size_t)k * 4, c->stream));
    if (R->nrows) {
      Timer tm(c, 24, (uint64_t)R->nrows * k);  // "ssp_rows_violations" (mfhip.hip: timing_kind)
      hipLaunchKernelGGL(k_rows_violations, g1(R->nrows, k), dim3(256), 0, c->stream, R->row_ptr(), R->wire(), R->coef(), R->nrows, d_bits, bs, d_count, d_first);
    }
    HIP_TRY(c, hipGetLastError());
    HIP_TRY(c, hipMemcpyAsync(h_count + s0, d_count, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
    if (h_first) HIP_TRY(c, hipMemcpyAsync(h_first + s0, d_first, (size_t)k * 4, hipMemcpyDeviceToHost, c->stream));
  }
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return MFH_OK;
}

}  // extern "C"
