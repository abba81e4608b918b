// raster_sums7.inc -- the end of a measuring kernel of R, G, B (K8's merge420_kernel<true>, K12's measure_tiles420_kernel), included into the kernel's body where every
// lane of the workgroup arrives with its uint32_t sse[3], worst[3] and count and the arguments `p` with p.out [7]: the lanes of a wave by __shfl_xor, the waves
// through LDS, then one 64-bit atomic per word and workgroup, out[2 c] += sse[c], out[2 c + 1] = max(.., worst[c]), out[6] += count. Integers: the same bits in
// every run. Text, not a function: called as a function the same instructions come out in another order, and both kernels then measured 0.1 - 0.9 % slower
// (profiles/raster_common_time.txt). K10's measure_tiles_kernel<C> reduces 2 C + 1 words of an array the same way, in its own words.
    __shared__ uint32_t s_part[kRasterThreads / 64][7];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
#pragma unroll
        for (int c = 0; c < 3; c++) {
            sse[c] += __shfl_xor(sse[c], o);
            worst[c] = max(worst[c], (uint32_t)__shfl_xor(worst[c], o));
        }
        count += __shfl_xor(count, o);
    }
    if (lane == 0) {
#pragma unroll
        for (int c = 0; c < 3; c++) s_part[wave][2 * c] = sse[c], s_part[wave][2 * c + 1] = worst[c];
        s_part[wave][6] = count;
    }
    __syncthreads();
    if (threadIdx.x < 7) {
        const bool is_max = threadIdx.x < 6 && (threadIdx.x & 1);
        unsigned long long v = 0;
#pragma unroll
        for (int w = 0; w < kRasterThreads / 64; w++) v = is_max ? max(v, (unsigned long long)s_part[w][threadIdx.x]) : v + s_part[w][threadIdx.x];
        if (v) {
            if (is_max) atomicMax(p.out + threadIdx.x, v);
            else atomicAdd(p.out + threadIdx.x, v);
        }
    }
