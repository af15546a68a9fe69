// TEST HARNESS ONLY (tests/test_dkg_verify_host.py).  Compiles the device headers of threshold_crypto_amd/csrc with g++ and
// exposes the Fr routines of the DKG verification entries (tc_dkg.h): Poly::evaluate, BivarPoly::row and the scalars of the
// combined values check.  Never linked into libtc_amd.so.  With -DDV_MAIN it is a stand-alone program (for a sanitizer
// build: g++ -fsanitize=address,undefined -DDV_MAIN) that runs every routine once over fixed inputs.
#include "tc_dkg.h"
#include <stdio.h>
#include <string.h>
#include <vector>
using namespace tc;

extern "C" {
// out = Poly(coeff).evaluate(x); coeff: n x 32 B LE, x: 32 B LE.  Returns the job status.
int dv_fr_poly_evaluate(const uint8_t* coeff, size_t n, const uint8_t* x_le32, uint8_t* out32) {
  std::vector<uint32_t> mont(n * 8 + 8);
  std::vector<uint8_t> valid(n + 1);
  for (size_t k = 0; k < n; k++) valid[k] = fr_mont_from_le32(coeff + k * 32, mont.data() + k * 8) ? 1 : 0;
  return job_fr_poly_evaluate(mont.data(), valid.data(), n, x_le32, out32);
}
// out[i] = BivarPoly::row(x)[i], status[i]; coeff: (degree+1)(degree+2)/2 x 32 B LE in coeff_pos order
void dv_bivar_poly_row(const uint8_t* coeff, size_t degree, uint64_t x, uint8_t* out, uint8_t* status) {
  const size_t n = degree + 1;
  std::vector<uint32_t> mont(n * n * 8);
  std::vector<uint8_t> valid(n * n);
  for (size_t t = 0; t < n * n; t++) valid[t] = fr_mont_from_le32(coeff + bivar_coeff_pos(t / n, t % n) * 32, mont.data() + t * 8) ? 1 : 0;
  for (size_t i = 0; i < n; i++) status[i] = job_bivar_poly_row(mont.data(), valid.data(), degree, i, x, out + i * 32);
}
static void key_words(const uint8_t* seed32, uint32_t* key) {
  for (int w = 0; w < 8; w++)
    key[w] = (uint32_t)seed32[4 * w] | ((uint32_t)seed32[4 * w + 1] << 8) | ((uint32_t)seed32[4 * w + 2] << 16) | ((uint32_t)seed32[4 * w + 3] << 24);
}
uint64_t dv_rlc_rho(const uint8_t* seed32, uint64_t counter) {
  uint32_t key[8];
  key_words(seed32, key);
  return dkg_rlc_rho(key, counter);
}
// the degree + 2 scalars of job j as 32 B LE each; returns 1 when every value is canonical
int dv_rlc_scalars(const uint8_t* seed32, size_t j, size_t n, size_t degree, const uint64_t* xs, const uint8_t* vals, uint8_t* out) {
  uint32_t key[8];
  key_words(seed32, key);
  std::vector<uint32_t> w((degree + 2) * 8);
  const bool ok = job_dkg_rlc_scalars(key, j, n, degree, xs, vals, w.data());
  for (size_t t = 0; t < w.size(); t++)
    for (int b = 0; b < 4; b++) out[4 * t + b] = (uint8_t)(w[t] >> (8 * b));
  return ok ? 1 : 0;
}
}

#if defined(DV_MAIN)
int main() {
  const size_t degree = 7, n = 5;
  std::vector<uint8_t> coeff((degree + 1) * (degree + 2) / 2 * 32), out((degree + 2) * 32), st(degree + 1), vals(n * 32);
  for (size_t i = 0; i < coeff.size(); i++) coeff[i] = (i % 32 == 31) ? 0 : (uint8_t)(i * 37 + 11);
  for (size_t i = 0; i < vals.size(); i++) vals[i] = (i % 32 == 31) ? 0 : (uint8_t)(i * 101 + 3);
  uint8_t x[32] = {5}, seed[32] = {1, 2, 3};
  const uint64_t xs[n] = {0, 1, 2, 5, ~0ull};
  int rc = dv_fr_poly_evaluate(coeff.data(), degree + 1, x, out.data());
  rc |= dv_fr_poly_evaluate(coeff.data(), 0, x, out.data());
  dv_bivar_poly_row(coeff.data(), degree, ~0ull, out.data(), st.data());
  for (size_t i = 0; i <= degree; i++) rc |= st[i];
  rc |= dv_rlc_scalars(seed, 3, n, degree, xs, vals.data(), out.data()) ? 0 : 1;
  rc |= (dv_rlc_rho(seed, 7) & 1) ? 0 : 1;
  printf("dkg_verify_host: %s\n", rc ? "FAILED" : "ok");
  return rc;
}
#endif
