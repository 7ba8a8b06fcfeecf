// The lab entry point (tools/lab_csr.py): product launch, clocked copies, probes, setups.
// variant 0: the product launch; 1: the clocked copy (clk: 64 B per wave, 4 waves per block)
extern "C" __attribute__((visibility("default"))) int k2h_lab_csr(int variant, const void* bytes,
                                                                  const uint64_t* offsets, uint64_t n, uint64_t* h1,
                                                                  void* clk, void* stream) {
  using namespace k2h;
  hipStream_t st = (hipStream_t)stream;
  const uint64_t seed = kSeedBuiltin;
  if (variant == 0) return (int)launch_csr_tile(bytes, offsets, n, seed, h1, nullptr, st, nullptr);
  const SpadTable t = make_spad(seed);
  const unsigned g = (unsigned)((n + kTileKeys - 1) / kTileKeys);
  const uint8_t* b = (const uint8_t*)bytes;
  uint32_t* c = (uint32_t*)clk;
  // 11-14: probes (11: one block per CU via 80 KiB of extra dynamic LDS; 12: setup at
  // priority 0; 13: the bare chain (wrong hashes); 14: 13 at one block per CU)
  // 2: the split-chain pair walk; 15 / 16: probes 13 / 14 over the split-chain step
  if (variant == 1) lab::csr_clock_kernel<1, 0><<<g, 256, 0, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 2) lab::csr_clock_kernel<1, 2><<<g, 256, 0, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 11) lab::csr_clock_kernel<1, 0><<<g, 256, 80 * 1024, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 12) lab::csr_clock_kernel<0, 0><<<g, 256, 0, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 13) lab::csr_clock_kernel<1, 1><<<g, 256, 0, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 14) lab::csr_clock_kernel<1, 1><<<g, 256, 80 * 1024, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 15) lab::csr_clock_kernel<1, 3><<<g, 256, 0, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 16) lab::csr_clock_kernel<1, 3><<<g, 256, 80 * 1024, st>>>(b, offsets, n, t, h1, c);
  // 3 / 4: the shorter setups of lab_csr_setup.inc (4 includes its order pre-pass)
  else if (variant == 3) lab::csr_setup_kernel<1><<<g, 256, 0, st>>>(b, offsets, n, t, h1, nullptr, c);
  else if (variant == 5) lab::csr_split_setup_kernel<true><<<g, 256, 0, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 6) lab::csr_split_setup_kernel<false><<<g, 256, 0, st>>>(b, offsets, n, t, h1, c);
  else if (variant == 4) {
    static uint16_t* order = nullptr;
    static uint64_t cap = 0;
    if (cap < n) {
      if (order) (void)hipFree(order);
      if (hipMalloc((void**)&order, n * sizeof(uint16_t)) != hipSuccess) return -2;
      cap = n;
    }
    lab::csr_order_kernel<<<g, 256, 0, st>>>(offsets, n, order);
    lab::csr_setup_kernel<2><<<g, 256, 0, st>>>(b, offsets, n, t, h1, order, c);
  } else return -1;
  return (int)hipGetLastError();
  return -1;
}
