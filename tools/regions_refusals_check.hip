// Host-only check of the regional prompts' refusals (k5_dit_set_regions and the regions' branches of sample_refusals in
// kandinsky-5_amd/csrc/engine.hip) under AddressSanitizer and UBSan: neither makes a HIP call, so both run on a machine without a GPU, on a
// default-constructed handle, with fake non-null device pointers that are never dereferenced and real host arrays for what the host reads.  The
// engine source is included whole (the handle's struct lives there); the other objects of the library are linked as built:
//
//   python kandinsky-5_amd/build.py
//   hipcc --offload-arch=gfx950 -O1 -g -std=c++17 -w -I include -I kandinsky-5_amd/csrc -Xarch_host -fsanitize=address,undefined \
//       -c tools/regions_refusals_check.hip -o /tmp/regions_refusals_check.o
//   hipcc --offload-arch=gfx950 -fsanitize=address,undefined /tmp/regions_refusals_check.o \
//       $(ls kandinsky-5_amd/build/*.o | grep -v /engine.o) -ldl -o /tmp/regions_refusals_check
//   /tmp/regions_refusals_check          (prints one line per case; exit status 0 = every status and message as expected)
#include "engine.hip"

#include <cmath>
#include <cstdio>

static int failures = 0;

static void expect(const char* what, int got, int want, const char* message) {
  const bool ok = got == want && (!message || strstr(k5_last_error(), message));
  printf("%-52s status %d %s%s\n", what, got, ok ? "ok" : "UNEXPECTED: ", ok ? "" : k5_last_error());
  failures += !ok;
}

static void expect_state(k5_dit* d, const char* what, int on, int R) {
  int got_on = -1, got_R = -1;
  long long n = -1;
  const int st = k5_dit_regions_state(d, &got_on, &got_R, &n, 0);
  const bool ok = st == K5_OK && got_on == on && got_R == R && n == 0;
  printf("%-52s on %d R %d %s\n", what, got_on, got_R, ok ? "ok" : "UNEXPECTED");
  failures += !ok;
}

int main() {
  k5_dit* d = new k5_dit();
  d->cfg.in_visual_dim = d->cfg.out_visual_dim = 16;
  d->cfg.patch_size[0] = 1; d->cfg.patch_size[1] = 2; d->cfg.patch_size[2] = 2;
  const int T = 3, H = 8, W = 12;
  const uintptr_t base = 0x10000000;                       // fake device addresses, never dereferenced
  auto at = [](uintptr_t p) { return reinterpret_cast<float*>(p); };
  int32_t pos[6] = {0, 1, 2, 3, 4, 5};
  k5_text_cond conds[9];
  for (auto& c : conds) { c = k5_text_cond{}; c.text_embed = at(base); c.pooled_embed = nullptr; c.text_len = 6; c.text_rope_pos = pos; }
  const float* masks = at(base + 0x100000);

  expect("null handle", k5_dit_set_regions(nullptr, conds, 2, masks, T, H, W, 0.f), K5_ERR_ARG, "null handle");
  expect("R = 9", k5_dit_set_regions(d, conds, 9, masks, T, H, W, 0.f), K5_ERR_ARG, "R must be 1..8 (got 9)");
  expect("R = -1", k5_dit_set_regions(d, conds, -1, masks, T, H, W, 0.f), K5_ERR_ARG, "R must be 1..8");
  expect("base_weight -0.5", k5_dit_set_regions(d, conds, 2, masks, T, H, W, -0.5f), K5_ERR_ARG, "base_weight must be in [0, 1]");
  expect("base_weight 1.5", k5_dit_set_regions(d, conds, 2, masks, T, H, W, 1.5f), K5_ERR_ARG, "base_weight must be in [0, 1]");
  expect("base_weight NaN", k5_dit_set_regions(d, conds, 2, masks, T, H, W, std::nanf("")), K5_ERR_ARG, "base_weight must be in [0, 1]");
  expect("masks NULL", k5_dit_set_regions(d, conds, 2, nullptr, T, H, W, 0.f), K5_ERR_ARG, "masks is NULL");
  expect("masks misaligned", k5_dit_set_regions(d, conds, 2, at(base + 2), T, H, W, 0.f), K5_ERR_ARG, "not 4-byte aligned");
  expect("H not divisible by the patch", k5_dit_set_regions(d, conds, 2, masks, T, 7, W, 0.f), K5_ERR_ARG, "(3, 7, 12) must be positive and divisible by the patch (1, 2, 2)");
  expect("W not divisible by the patch", k5_dit_set_regions(d, conds, 2, masks, T, H, 11, 0.f), K5_ERR_ARG, "divisible by the patch");
  expect("T = 0", k5_dit_set_regions(d, conds, 2, masks, 0, H, W, 0.f), K5_ERR_ARG, "must be positive");
  conds[1].text_len = 0;
  expect("region 1, text_len 0", k5_dit_set_regions(d, conds, 2, masks, T, H, W, 0.f), K5_ERR_ARG, "region 1: text_len must be >= 1 (got 0)");
  conds[1].text_len = 6; conds[1].text_embed = nullptr;
  expect("region 1, text_embed NULL", k5_dit_set_regions(d, conds, 2, masks, T, H, W, 0.f), K5_ERR_ARG, "region 1 needs text_embed and text_rope_pos");
  conds[1].text_embed = at(base); conds[1].text_rope_pos = nullptr;
  expect("region 1, text_rope_pos NULL", k5_dit_set_regions(d, conds, 2, masks, T, H, W, 0.f), K5_ERR_ARG, "region 1 needs text_embed and text_rope_pos");
  conds[1].text_rope_pos = pos;
  expect("only the first R entries are read", k5_dit_set_regions(d, conds, 1, masks, T, H, W, 0.f), K5_OK, nullptr);
  k5_dit_set_regions(d, nullptr, 0, nullptr, 0, 0, 0, 0.f);
  expect_state(d, "nothing of the refused calls stuck", 0, 0);

  expect("R = 8, base_weight 1", k5_dit_set_regions(d, conds, 8, masks, T, H, W, 1.f), K5_OK, nullptr);
  expect_state(d, "set", 1, 8);
  expect("a refused call ...", k5_dit_set_regions(d, conds, 2, masks, T, H, W, 2.f), K5_ERR_ARG, "base_weight");
  expect_state(d, "... leaves what was set", 1, 8);
  expect("R = 0 clears", k5_dit_set_regions(d, conds, 0, masks, T, H, W, 0.f), K5_OK, nullptr);
  expect_state(d, "cleared", 0, 0);
  expect("R = 2", k5_dit_set_regions(d, conds, 2, masks, T, H, W, 0.25f), K5_OK, nullptr);
  expect("NULL clears, whatever the rest", k5_dit_set_regions(d, nullptr, 5, nullptr, -1, -1, -1, 9.f), K5_OK, nullptr);
  expect_state(d, "cleared", 0, 0);
  expect("state of a null handle", k5_dit_regions_state(nullptr, nullptr, nullptr, nullptr, 0), K5_ERR_ARG, "null handle");

  // the sampler's refusals with regions set
  float sigmas[5] = {1.0f, 0.75f, 0.5f, 0.25f, 0.0f};
  k5_sample_args a{};
  a.fwd.T = T; a.fwd.H = H; a.fwd.W = W;
  a.latent = at(base + 0x200000); a.sigmas = sigmas; a.num_steps = 4; a.guidance_weight = 5.0f;
  auto run = [&](const k5_sample_windows_args* w) { g_err[0] = 0; return sample_refusals(d, w ? &w->sample : &a, nullptr, nullptr, w, "check"); };
  float weights[2 * 3] = {1, 1, 1, 1, 1, 1};
  int starts[2] = {0, 2};
  k5_sample_windows_args w{};
  w.sample = a; w.weights = weights; w.starts = starts; w.nwin = 2; w.total_T = 5;
  expect("no regions: a sample of any shape", run(nullptr), K5_OK, nullptr);
  expect("no regions: windows", run(&w), K5_OK, nullptr);
  expect("regions of the sample's shape", k5_dit_set_regions(d, conds, 2, masks, T, H, W, 0.f), K5_OK, nullptr);
  expect("sample of the masks' shape", run(nullptr), K5_OK, nullptr);
  expect("windows with regions", run(&w), K5_ERR_STATE, "regional prompts are set (k5_dit_set_regions): the masks cover the clip, a context window sees a slice");
  a.fwd.W = 16;
  expect("sample of another W", run(nullptr), K5_ERR_ARG, "the masks are (3, 8, 12), this sample is (3, 8, 16)");
  a.fwd.W = W; a.fwd.T = 5;
  expect("sample of another T", run(nullptr), K5_ERR_ARG, "the masks are (3, 8, 12), this sample is (5, 8, 12)");
  a.fwd.T = T; a.fwd.H = 16;
  expect("sample of another H", run(nullptr), K5_ERR_ARG, "the masks are (3, 8, 12), this sample is (3, 16, 12)");
  a.fwd.H = H;
  k5_dit_set_regions(d, nullptr, 0, nullptr, 0, 0, 0, 0.f);
  a.fwd.W = 16;
  expect("cleared: a sample of any shape again", run(nullptr), K5_OK, nullptr);
  expect("cleared: windows again", run(&w), K5_OK, nullptr);
  delete d;
  printf("%d unexpected\n", failures);
  return failures ? 1 : 0;
}
