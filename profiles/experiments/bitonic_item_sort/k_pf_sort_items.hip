// k_pf_sort_items - the bitonic item sort of the pileup partition sort, retired.  Kernel text as it stood in csrc/fold_partition.h
// (selected by XCK_PILEUP_ITEM_SORT=bitonic, launched with one block of PS_THREADS per item where k_pf_radix_items is launched now).
// Not built: it needs PF_CAP_MAX and the counter word CTR_ITEM_OVER (then the literal 7) of fold_partition.h.  See README.md.
constexpr int PS_CAP = PF_CAP_MAX, PS_THREADS = 256;
__global__ __launch_bounds__(PS_THREADS) void k_pf_sort_items(unsigned long long* __restrict__ keys, uint64_t* __restrict__ vals, const uint32_t* __restrict__ item_off, uint32_t* __restrict__ ctr) {
    // Bitonic network on (key, value) in LDS.  Every wave owns a quarter of the array: the stages whose partner distance stays inside
    // a quarter are run by that wave alone, in lock step, without block barriers (63 of the 66 stages of a 2048-pair item); only
    // the three stages that pair elements of different quarters meet at a barrier.  (A barrier per stage: 67 us per item, 1.9 ms
    // for the 29 k items of configs[2].)
    __shared__ unsigned long long sk[PS_CAP];
    __shared__ unsigned long long sv[PS_CAP];
    const uint32_t off = item_off[blockIdx.x], n = item_off[blockIdx.x + 1] - off;
    if (n < 2) return;
    if (n > (uint32_t)PS_CAP) { if (threadIdx.x == 0) ctr[7] = 1u; return; }
    uint32_t N2 = 2; while (N2 < n) N2 <<= 1;
    for (uint32_t i = threadIdx.x; i < N2; i += PS_THREADS) { sk[i] = i < n ? keys[off + i] : ~0ull; sv[i] = i < n ? vals[off + i] : ~0ull; }
    const uint32_t wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t SEG = max(N2 / (PS_THREADS / 64), 128u);                // elements of a wave's segment (a power of two, >= 2 per lane)
    const bool wave_on = wave * SEG < N2;
    auto cmpx = [&](uint32_t p, uint32_t j, uint32_t k) {                 // pair number p of stage (k, j)
        const uint32_t i = ((p & ~(j - 1)) << 1) | (p & (j - 1)), x = i | j;
        const unsigned long long ka = sk[i], kb = sk[x], va = sv[i], vb = sv[x];
        const bool gt = ka > kb || (ka == kb && va > vb);
        if (gt == ((i & k) == 0)) { sk[i] = kb; sk[x] = ka; sv[i] = vb; sv[x] = va; }
    };
    __syncthreads();
    for (uint32_t k = 2; k <= N2; k <<= 1)
        for (uint32_t j = k >> 1; j > 0; j >>= 1) {
            if (j >= SEG) {                                               // partners in different segments: the whole block, between barriers
                __syncthreads();
                for (uint32_t p = threadIdx.x; p < N2 / 2; p += PS_THREADS) cmpx(p, j, k);
                __syncthreads();
            } else {
                if (wave_on) for (uint32_t p = lane; p < min(SEG, N2) / 2; p += 64) cmpx(wave * (SEG / 2) + p, j, k);
                asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");        // this wave's exchanges have landed before its next stage reads
            }
        }
    __syncthreads();
    for (uint32_t i = threadIdx.x; i < n; i += PS_THREADS) { keys[off + i] = sk[i]; vals[off + i] = sv[i]; }
}
