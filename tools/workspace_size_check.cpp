// Host-only check of the workspace arithmetic at large geometry (whisperseg-large: d 1280, 20 heads, 32 + 32 layers, ffn 5120, vocab
// 51865) for 500 and 1500 encoder positions, up to 1024 slots: wseg_model_create and wseg_workspace_bytes* only fill host structures, so
// this runs without a GPU.  Build it together with the library's sources under the host sanitizer and run it:
//
//   hipcc --offload-arch=gfx950 -O1 -std=c++17 -Xarch_host -fsanitize=undefined -Xarch_host -fno-sanitize-recover=undefined \
//         tools/workspace_size_check.cpp whisperseg_amd/csrc/*.hip -o workspace_size_check && ./workspace_size_check
//
// It prints one line per (mode, positions, slots, beams) and fails when a size is zero, not monotone in the slot count, or when 1500
// positions do not cost more than 500.
#include <cstdio>
#include <cstdlib>
#include "../include/wseg.h"

int main() {
  int bad = 0;
  for (int dtype = WSEG_F32; dtype <= WSEG_F16M6; ++dtype) {
    size_t at500[2][3] = {};
    const int pos[2] = {500, 1500};
    for (int pi = 0; pi < 2; ++pi) {
      wseg_model_config c = {};
      c.d_model = 1280; c.n_heads = 20; c.enc_layers = 32; c.dec_layers = 32; c.ffn = 5120; c.vocab = 51865; c.n_mels = 80;
      c.spec_cols = 2 * pos[pi]; c.enc_positions = pos[pi]; c.dec_positions = 448; c.dtype = dtype;
      wseg_model* m = nullptr;
      if (wseg_model_create(&c, &m) != WSEG_OK) { std::printf("create failed: %s\n", wseg_last_error()); return 1; }
      const int beams[2] = {4, 8}, slots[3] = {1, 256, 1024};
      for (int bi = 0; bi < 2; ++bi) {
        size_t prev = 0;
        for (int si = 0; si < 3; ++si) {
          const size_t a = wseg_workspace_bytes(m, slots[si], beams[bi], 448);
          const size_t b = wseg_workspace_bytes_kv(m, slots[si], beams[bi], 448, 448);
          std::printf("dtype %d positions %4d slots %4d beams %d: %zu bytes (%.1f GiB), full K/V pool %zu\n", dtype, pos[pi], slots[si], beams[bi], a,
                      (double)a / (1ull << 30), b);
          if (a == 0 || b < a || a <= prev) { std::printf("  ^ not positive / monotone\n"); ++bad; }
          if (pi == 0) at500[bi][si] = a;
          else if (a <= at500[bi][si]) { std::printf("  ^ 1500 positions must cost more than 500\n"); ++bad; }
          prev = a;
        }
      }
      wseg_model_destroy(m);
    }
  }
  std::printf(bad ? "FAILED: %d\n" : "ok\n", bad);
  return bad ? 1 : 0;
}
