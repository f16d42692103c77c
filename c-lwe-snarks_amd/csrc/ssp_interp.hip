// ssp_interp.hip -- mfh_ssp_from_rows: a constraint system given row by row (evaluation form) written as the dense device SSP (coefficient form).
//
// Points r_j = j + 2, j = 0 .. n - 1 (n = d - 1).  t(x) = prod_j (x - r_j): monic of degree d - 1, no root at +-1 (the exact-division path of poly.hip
// needs deg t = d - 1 and t a unit modulo x^N - 1, whose only roots in F_p are +-1).  v_i is the interpolant of its column: with the Lagrange weights
// w_j = 1 / prod_{l != j} (r_j - r_l) = 1 / ((-1)^(n-1-j) j! (n-1-j)!) and Q_j = t / (x - r_j),
//     v_i(x) = sum_j V_ij w_j Q_j(x),     q_{j,d-1} = 0,  q_{j,k-1} = t_k + r_j q_{j,k}   (synthetic division of t by x - r_j).
// So the SSP is a sparse (wires x rows) by dense (rows x coefficients) product mod p; the result is canonical residues, exact in any summation order.
//
// Per context (t and the weights depend on d alone, and d is fixed per context): t and the weights from the tree of t of the row SSP (ssp_rows.hip), and a seed
// table seeds[j][b] = q_{j, (b+1) G - 1}: the value of the recurrence at the top of every G-coefficient sub-tile, so that a thread regenerates one sub-tile's
// q_{j,k} in registers from one load.  Per call: the rows are sorted into wire columns on the host (c_ij = V_ij w_j, O(nnz)), cut into parts of at most CH
// nonzeros (load balance by nonzeros: v_0 carries every booleanity row, every gate row and the padding), and one launch writes every slot; parts of a cut
// column go to scratch and a second launch sums them.
#include <algorithm>
#include <vector>

#include "ctx.hpp"
#include "p32.hpp"

namespace {

constexpr int IG = 32;            // coefficients per thread (one sub-tile): 32 uint64 accumulators + 32 t words in registers
constexpr uint32_t IWG = 256;     // threads per workgroup of the gather launch
constexpr uint32_t CH_MIN = 256;  // nonzeros per part, at least (parts of a cut column go through scratch)
constexpr uint32_t MAX_CUT = 512; // ... and more when nnz / CH_MIN would exceed this: scratch <= 2 * MAX_CUT * d words

// ---- seeds.  Over sub-tile b the recurrence is affine: q_{bG-1} = r^G q_{top(b)} + L_b, with L_b its G steps from 0 (top(b) = bG + G - 1).
__global__ __launch_bounds__(256) void k_seed_local(const uint32_t *__restrict__ tpad, uint32_t n, uint32_t NB, uint32_t *__restrict__ seeds) {
  const uint64_t idx = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (idx >= (uint64_t)n * NB) return;
  const uint32_t j = (uint32_t)(idx / NB), b = (uint32_t)(idx % NB);
  const uint64_t r = j + 2;
  uint32_t q = 0;
#pragma unroll
  for (int s = IG - 1; s >= 0; s--) q = red_p32(r * q + tpad[(size_t)b * IG + s]);
  seeds[idx] = q;
}
// ... then per row, from the top (q_{Dp-1} = 0): seed_b = q_{top(b)}, seed_{b-1} = r^G seed_b + L_b (in place: L_b is read before seed_b is written)
__global__ __launch_bounds__(256) void k_seed_scan(uint32_t n, uint32_t NB, uint32_t *__restrict__ seeds) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  uint32_t rg = 1;
  for (int s = 0; s < IG; s++) rg = red_p32((uint64_t)rg * (j + 2));
  uint32_t *row = seeds + (size_t)j * NB, carry = 0;
  for (uint32_t b = NB; b-- > 0;) {
    const uint32_t l = row[b];
    row[b] = carry;
    carry = red_p32((uint64_t)rg * carry + l);
  }
}

// ---- the gather product.  parts[p] = {first nonzero, count, destination slot or scratch row, 1 = scratch}; nz[e] = {row j, c = V_ij w_j}.
// Workgroup (p, g): sub-tiles b = g * 256 + tid, coefficients [bG, bG + G) per thread; every lane of a wave walks the same nonzeros (wave-uniform
// loads), regenerating q_{j,k} from seeds[j][b] downwards.  The results go out through LDS so that each store instruction of a wave writes 1 KB
// contiguous.  A part without nonzeros writes zeros (empty wires).
__global__ __launch_bounds__(IWG) void k_interp(const uint2 *__restrict__ nz, const uint4 *__restrict__ parts, uint32_t wg_per_part,
                                                const uint32_t *__restrict__ seeds, uint32_t NB, const uint32_t *__restrict__ tpad, uint32_t d, int vec4,
                                                uint32_t *__restrict__ ssp, uint32_t *__restrict__ scratch) {
  __shared__ uint32_t lds[IWG / 64][64 * (IG + 1)];
  const uint32_t part = blockIdx.x / wg_per_part, g = blockIdx.x % wg_per_part;
  const uint4 pd = parts[part];
  const uint32_t b = g * IWG + threadIdx.x;
  const uint32_t bs = b < NB ? b : NB - 1;  // lanes past the last sub-tile compute on a valid one and store nothing
  uint32_t tv[IG];
#pragma unroll
  for (int s = 0; s < IG; s++) tv[s] = tpad[(size_t)bs * IG + s];
  uint64_t acc[IG];
#pragma unroll
  for (int s = 0; s < IG; s++) acc[s] = 0;
  const uint2 *z = nz + pd.x;
  uint32_t qn = pd.y ? seeds[(size_t)z[0].x * NB + bs] : 0;
  for (uint32_t e = 0; e < pd.y; e++) {
    const uint2 ze = z[e];
    uint32_t q = qn;
    if (e + 1 < pd.y) qn = seeds[(size_t)z[e + 1].x * NB + bs];  // next row's seed in flight while this one is walked
    const uint64_t r = ze.x + 2, cf = ze.y;
#pragma unroll
    for (int s = IG - 1; s >= 0; s--) {
      acc[s] += fold1(cf * q);
      if (s) q = red_p32(r * q + tv[s]);
    }
  }
  const uint32_t lane = threadIdx.x & 63;
  uint32_t *L = lds[threadIdx.x >> 6];
#pragma unroll
  for (int s = 0; s < IG; s++) L[lane * (IG + 1) + s] = red_p32(acc[s]);
  __syncthreads();
  uint32_t *dst = (pd.w ? scratch : ssp) + (size_t)pd.z * d;
  const uint32_t k0 = (g * IWG + (threadIdx.x & ~63u)) * IG;  // the wave's first coefficient
#pragma unroll
  for (int it = 0; it < IG / 4; it++) {
    const uint32_t o = it * 256 + lane * 4, src = (o / IG) * (IG + 1) + o % IG;
    const uint32_t k = k0 + o;
    if (vec4 && k + 3 < d) {
      *reinterpret_cast<uint4 *>(dst + k) = make_uint4(L[src], L[src + 1], L[src + 2], L[src + 3]);
    } else {
      for (int u = 0; u < 4; u++)
        if (k + u < d) dst[k + u] = L[src + u];
    }
  }
}
// columns cut into several parts: splits[y] = {slot, first scratch row, parts}
__global__ __launch_bounds__(256) void k_interp_sum(const uint4 *__restrict__ splits, const uint32_t *__restrict__ scratch, uint32_t d,
                                                    uint32_t *__restrict__ ssp) {
  const uint32_t k = blockIdx.x * blockDim.x + threadIdx.x;
  if (k >= d) return;
  const uint4 sp = splits[blockIdx.y];
  uint64_t acc = 0;
  for (uint32_t q = 0; q < sp.z; q++) acc += scratch[(size_t)(sp.y + q) * d + k];
  ssp[(size_t)sp.x * d + k] = red_p32(acc);
}

}  // namespace

// what mfh_ssp_from_rows keeps per context (the seeds depend on d alone)
struct SspInterp {
  uint32_t NB = 0;               // sub-tiles of G coefficients: Dp = NB * G >= d
  uint32_t *seeds = nullptr;     // n * NB words
  DevBuf buf;                    // per call: nonzeros | parts | splits
  DevBuf scratch;                // per call: the parts of cut columns
};

void ssp_interp_free(mfh_ctx *c) {
  SspInterp *s = c->interp;
  if (!s) return;
  if (s->seeds) hipFree(s->seeds);
  dev_free(s->buf);
  dev_free(s->scratch);
  delete s;
  c->interp = nullptr;
}

// the seed table from t (Dp words, zero-padded)
static int interp_prepare(mfh_ctx *c, const uint32_t *tpad) {
  if (c->interp && c->interp->seeds) return MFH_OK;
  if (!c->interp) c->interp = new SspInterp();
  SspInterp *s = c->interp;
  const uint32_t d = c->P.d, n = d - 1;
  s->NB = (d + IG - 1) / IG;
  if (hipMalloc((void **)&s->seeds, (size_t)n * s->NB * 4) != hipSuccess) {
    (void)hipGetLastError();
    s->seeds = nullptr;
    c->err = "mfh_ssp_from_rows: no memory for the seed table";
    return MFH_ENOMEM;
  }
  const uint64_t nseed = (uint64_t)n * s->NB;
  hipLaunchKernelGGL(k_seed_local, dim3((uint32_t)((nseed + 255) / 256)), dim3(256), 0, c->stream, tpad, n, s->NB, s->seeds);
  hipLaunchKernelGGL(k_seed_scan, dim3((n + 255) / 256), dim3(256), 0, c->stream, n, s->NB, s->seeds);
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) {
    hipFree(s->seeds);
    s->seeds = nullptr;
    c->err = "mfh_ssp_from_rows: building the seed table failed";
    return MFH_EDEVICE;
  }
  return MFH_OK;
}

int mfh_ssp_from_rows(mfh_ctx *c, uint32_t nrows, const uint32_t *h_row_ptr, const uint32_t *h_wire, const uint32_t *h_coef, uint32_t *d_ssp) {
  if (!c || !h_row_ptr || !d_ssp) return MFH_EINVAL;
  if (int rc = ssp_rows_check(c, "mfh_ssp_from_rows", nrows, h_row_ptr, h_wire, h_coef)) return rc;
  const uint32_t d = c->P.d, m = c->P.m, n = d - 1;
  std::vector<uint32_t> cnt(m, 0);
  for (uint32_t e = h_row_ptr[0]; e < h_row_ptr[nrows]; e++)
    if (h_coef[e]) cnt[h_wire[e]]++;
  HIP_TRY(c, hipSetDevice(c->device));
  const uint32_t *tpad, *w;
  if (int rc = ssp_rows_tree(c, "mfh_ssp_from_rows", tpad, w)) return rc;
  if (int rc = interp_prepare(c, tpad)) return rc;
  SspInterp *s = c->interp;
  cnt[0] += n - nrows;  // padding rows: v_0(r_j) = 1

  // wire columns, c_ij = V_ij w_j (duplicates stay separate entries: the sum adds them)
  std::vector<uint64_t> off(m + 1, 0);
  for (uint32_t i = 0; i < m; i++) off[i + 1] = off[i] + cnt[i];
  const uint64_t nnz = off[m];
  const uint64_t ch = std::max<uint64_t>(CH_MIN, (nnz + MAX_CUT - 1) / MAX_CUT);
  std::vector<uint32_t> parts_h, splits_h;  // uint4 records
  std::vector<std::pair<uint32_t, uint32_t>> whole;  // (count, wire) of the columns that are not cut
  uint32_t ncut = 0;
  for (uint32_t i = 0; i < m; i++) {
    if (cnt[i] <= ch) { whole.emplace_back(cnt[i], i); continue; }
    const uint32_t np = (uint32_t)((cnt[i] + ch - 1) / ch);
    splits_h.insert(splits_h.end(), {i + 1, ncut, np, 0});
    for (uint32_t q = 0; q < np; q++) {
      const uint64_t a = off[i] + q * ch, b = std::min<uint64_t>(off[i] + (q + 1) * ch, off[i + 1]);
      parts_h.insert(parts_h.end(), {(uint32_t)a, (uint32_t)(b - a), ncut + q, 1});
    }
    ncut += np;
  }
  std::stable_sort(whole.begin(), whole.end(), [](const std::pair<uint32_t, uint32_t> &x, const std::pair<uint32_t, uint32_t> &y) { return x.first > y.first; });
  for (auto &wc : whole) parts_h.insert(parts_h.end(), {(uint32_t)off[wc.second], wc.first, wc.second + 1, 0});  // heaviest first
  const uint32_t nparts = (uint32_t)(parts_h.size() / 4), nsplit = (uint32_t)(splits_h.size() / 4);

  const size_t nz_words = 2 * (size_t)nnz, bytes = (nz_words + parts_h.size() + splits_h.size()) * 4;
  std::vector<uint32_t> host(nz_words + parts_h.size() + splits_h.size());
  {
    std::vector<uint64_t> pos(off.begin(), off.end() - 1);
    for (uint32_t j = 0; j < nrows; j++)
      for (uint32_t e = h_row_ptr[j]; e < h_row_ptr[j + 1]; e++) {
        if (!h_coef[e]) continue;
        const uint64_t q = pos[h_wire[e]]++;
        host[2 * q] = j;
        host[2 * q + 1] = mulp(h_coef[e], w[j]);
      }
    for (uint32_t j = nrows; j < n; j++) {
      const uint64_t q = pos[0]++;
      host[2 * q] = j;
      host[2 * q + 1] = w[j];
    }
  }
  std::copy(parts_h.begin(), parts_h.end(), host.begin() + nz_words);
  std::copy(splits_h.begin(), splits_h.end(), host.begin() + nz_words + parts_h.size());
  if (int rc = work_reserve(c, s->buf, std::max<size_t>(bytes, 16))) return rc;
  if (ncut)
    if (int rc = work_reserve(c, s->scratch, (size_t)ncut * d * 4)) return rc;

  ssp_images_stale(c);  // derived images of the SSP are stale
  HIP_TRY(c, hipMemcpyAsync(s->buf.p, host.data(), bytes, hipMemcpyHostToDevice, c->stream));
  const uint2 *d_nz = s->buf.as<const uint2>();
  const uint4 *d_parts = (const uint4 *)(s->buf.as<uint32_t>() + nz_words), *d_splits = d_parts + nparts;
  HIP_TRY(c, hipMemcpyAsync(d_ssp, tpad, (size_t)d * 4, hipMemcpyDeviceToDevice, c->stream));  // slot 0 = t
  HIP_TRY(c, hipMemsetAsync(d_ssp + (size_t)(m + 1) * d, 0, (size_t)2 * d * 4, c->stream));  // slots m + 1, m + 2
  {
    Timer tm(c, 15, nnz);
    const uint32_t wg_per_part = (s->NB + IWG - 1) / IWG;
    const int vec4 = d % 4 == 0 && ((uintptr_t)d_ssp & 15) == 0;
    hipLaunchKernelGGL(k_interp, dim3(nparts * wg_per_part), dim3(IWG), 0, c->stream, d_nz, d_parts, wg_per_part, (const uint32_t *)s->seeds, s->NB, tpad, d,
                       vec4, d_ssp, s->scratch.as<uint32_t>());
    if (nsplit) hipLaunchKernelGGL(k_interp_sum, dim3((d + 255) / 256, nsplit), dim3(256), 0, c->stream, d_splits, s->scratch.as<const uint32_t>(), d, d_ssp);
  }
  // (host holds the staged rows: the copy must have run before it goes out of scope)
  if (hipGetLastError() != hipSuccess || hipStreamSynchronize(c->stream) != hipSuccess) { c->err = "mfh_ssp_from_rows: launch failed"; return MFH_EDEVICE; }
  return MFH_OK;
}
