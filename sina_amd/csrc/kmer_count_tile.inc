// The count kernels' work on one tile of references (kmer.hip: kmer_count_kernel, kmer_count_long_kernel), included
// in the body of their tile loops -- text, not a function: the fast kernel's code object is the one it was before the
// long kernel came to share this.  Reads a, tid, lane, hist, cur, end, dtop, nk, nd, next_kmer, tile_lo, tile_hi; leaves
// the tile's counters in hist[], every thread behind a barrier.
        for (uint32_t i = tid; i < kTileRefs / 8; i += kCountThreads) reinterpret_cast<uint4 *>(hist)[i] = uint4{0u, 0u, 0u, 0u};
        if (tid == 0) next_kmer = 0;
        __syncthreads();
        for (uint32_t guard = 0; guard < (1u << 22); guard++) {
            uint32_t i = 0;
            if (lane == 0) i = atomicAdd(&next_kmer, 1u);
            i = __builtin_amdgcn_readfirstlane(i);
            if (i >= nk) break;
            uint32_t c = cur[i];
            const uint32_t e = end[i];
            // First a probe of 64 postings, one per lane.  Most visits end here: 1250 of a query's ~1330 cursor lists
            // are short -- ~130 postings at 500 000 references, eight or so per tile -- and the wide loop below costs
            // such a visit a hundred instructions (the kernel is bound by instruction issue, not by the round trips:
            // 32 waves per CU hide those).  The lists are ascending: the postings of this tile are a prefix.
            {
                const uint32_t x = c + (uint32_t)lane;
                const uint32_t id = x < e ? a.idx_ids[x] : 0xFFFFFFFFu;
                const bool in = id < tile_hi;
                if (in) {
                    const uint32_t r = id - tile_lo;
                    atomicAdd(&hist[r >> 1], 1u << (16 * (r & 1)));
                }
                const uint32_t cnt = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(in));
                c += cnt;
                if (cnt < 64u) {
                    if (lane == 0) cur[i] = c;
                    continue;
                }
            }
            // kWide x 1 KiB in flight per wave: every lane reads four consecutive postings per load
            // (most postings sit in a few hundred long lists -- k-mers of conserved regions -- and
            // one wave streams each of them: bytes in flight are what bounds it)
            for (uint32_t g2 = 0; c < e && g2 < (1u << 22); g2++) {
                uint32_t id[kWide][4];
#pragma unroll
                for (int u = 0; u < kWide; u++) {
                    const uint32_t x = c + 4u * (uint32_t)lane + 256u * u;
                    if (x + 4u <= e) {
                        const uint32_t *src = a.idx_ids + x;  // (4-byte aligned: three dwords + one, or one 16-byte load)
                        id[u][0] = src[0];
                        id[u][1] = src[1];
                        id[u][2] = src[2];
                        id[u][3] = src[3];
                    } else {
#pragma unroll
                        for (int v = 0; v < 4; v++) id[u][v] = (x + v < e) ? a.idx_ids[x + v] : 0xFFFFFFFFu;
                    }
                }
                uint32_t cnt = 0;
#pragma unroll
                for (int u = 0; u < kWide; u++) {
#pragma unroll
                    for (int v = 0; v < 4; v++) {
                        if (id[u][v] < tile_hi) {
                            const uint32_t r = id[u][v] - tile_lo;
                            atomicAdd(&hist[r >> 1], 1u << (16 * (r & 1)));
                            cnt++;
                        }
                    }
                }
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) cnt += __shfl_xor(cnt, off);
                c += cnt;
                if (cnt < 256u * kWide) break;
            }
            if (lane == 0) cur[i] = c;
        }
        __syncthreads();
        // Dense k-mers: thread t owns the 32 references of bitmap word t of this tile and counts, for
        // each of them, in how many of the query's dense bitmaps its bit is set -- bit-sliced: the
        // planes hold one bit of all 32 counters each; eight bitmap words go in with seven carry-save
        // adders (ones / twos / fours) and one ripple of the resulting eights (7 operations per word,
        // no atomics, nothing but registers).
        if (nd) {
            // (the planes above the fours: as many as the query's number of dense k-mers has bits beyond three -- a
            // hundred bitmaps need four of the seven; the ripple and the unpacking below are compiled for each count)
            auto dense_path = [&](auto nhi_c) {
                constexpr int NHI = decltype(nhi_c)::value;
                // A bitmap's number and its row's address are the same for every thread: both stay on the scalar unit.
                // A wave fetches up to 64 numbers with one LDS read, a number per lane, padded to a multiple of eight
                // with the all-zero row (a.dense_zero: no branch per word); a word's load is the row's base in SGPRs
                // plus my_word, the loop-invariant byte offset of this thread's word in any row (32 bits: a row is at
                // most 2^29 bytes) -- one VGPR per word in flight, no vector multiply, no LDS wait in the body.
                const uint32_t my_word = 4u * ((tile_lo >> 5) + tid);
                const uint32_t row_bytes = 4u * a.dense_words;
                uint32_t ones = 0, twos = 0, fours = 0, hi[NHI > 0 ? NHI : 1] = {0};  // hi[p]: weight 8 << p
                auto csa = [](uint32_t &h, uint32_t &l, uint32_t x, uint32_t y, uint32_t z) {
                    const uint32_t u = x ^ y;
                    h = (x & y) | (u & z);
                    l = u ^ z;
                };
                for (uint32_t i0 = 0; i0 < nd; i0 += 64) {
                    const uint32_t n = min(nd - i0, 64u);
                    const uint32_t num = (uint32_t)lane < n ? *(dtop - (i0 + lane)) : a.dense_zero;
                    for (uint32_t j = 0; j < n; j += 8) {
                        uint32_t w[8];
                        uint32_t word = my_word;
                        asm("" : "+v"(word));  // (its 64-bit extension made here, where the loads' address selection sees it)
#pragma unroll
                        for (int u = 0; u < 8; u++) {
                            const uint32_t id = (uint32_t)__builtin_amdgcn_readlane((int)num, (int)(j + u));
                            // (the base pinned to SGPRs, in the global address space: the load takes it as its scalar base;
                            // folded into the thread's 64-bit address it costs a vector add and two VGPRs per word)
                            using global_bytes = const __attribute__((address_space(1))) char *;
                            global_bytes row_bits = (global_bytes)a.dense_bits + (uint64_t)id * row_bytes;
                            asm("" : "+s"(row_bits));
                            w[u] = *(const __attribute__((address_space(1))) uint32_t *)(row_bits + word);
                        }
                        uint32_t twosA, twosB, foursA, foursB, eights;
                        csa(twosA, ones, ones, w[0], w[1]);
                        csa(twosB, ones, ones, w[2], w[3]);
                        csa(foursA, twos, twos, twosA, twosB);
                        csa(twosA, ones, ones, w[4], w[5]);
                        csa(twosB, ones, ones, w[6], w[7]);
                        csa(foursB, twos, twos, twosA, twosB);
                        csa(eights, fours, fours, foursA, foursB);
                        uint32_t carry = eights;
#pragma unroll
                        for (int p = 0; p < NHI; p++) {
                            const uint32_t t2 = hi[p] & carry;
                            hi[p] ^= carry;
                            carry = t2;
                        }
                    }
                }
                // add my 32 counts to the tile's counters: words 16 t .. 16 t + 15 are mine alone now
                if constexpr (NHI <= 5) {
                    // counts below 256: four references at a time -- their bits of a plane are a nibble, one
                    // multiplication spreads the nibble's bits over the four bytes of a word (bit i to bit 8 i), the
                    // planes are or-ed in at their weights; two byte shuffles make the counters' two 16-bit pairs.
                    // (group g of lane l in step (g - l) mod 8, a 64-bit access each: the lanes of a wave spread over
                    // the LDS banks)
#pragma unroll 2
                    for (int gg = 0; gg < 8; gg++) {
                        const int g = (gg + lane) & 7;
                        const int b = 4 * g;
                        auto spread = [&](uint32_t plane) -> uint32_t { return (((plane >> b) & 0xFu) * 0x00204081u) & 0x01010101u; };
                        uint32_t acc = spread(ones) | (spread(twos) << 1) | (spread(fours) << 2);
#pragma unroll
                        for (int p = 0; p < NHI; p++) acc |= spread(hi[p]) << (3 + p);
                        uint2 *hw = reinterpret_cast<uint2 *>(&hist[16 * tid + 2 * g]);
                        uint2 v = *hw;
                        v.x += (acc & 0xFFu) | ((acc & 0xFF00u) << 8);
                        v.y += ((acc >> 16) & 0xFFu) | ((acc >> 24) << 16);
                        *hw = v;
                    }
                } else {
                    // (word j of lane l in step (j - l) mod 16: the lanes of a wave spread over the LDS banks)
#pragma unroll 4
                    for (int jj = 0; jj < 16; jj++) {
                        const int j = (jj + lane) & 15;
                        const int b0 = 2 * j, b1 = 2 * j + 1;
                        uint32_t cl = ((ones >> b0) & 1u) | (((twos >> b0) & 1u) << 1) | (((fours >> b0) & 1u) << 2);
                        uint32_t ch = ((ones >> b1) & 1u) | (((twos >> b1) & 1u) << 1) | (((fours >> b1) & 1u) << 2);
#pragma unroll
                        for (int p = 0; p < NHI; p++) {
                            cl |= ((hi[p] >> b0) & 1u) << (3 + p);
                            ch |= ((hi[p] >> b1) & 1u) << (3 + p);
                        }
                        hist[16 * tid + j] += cl | (ch << 16);
                    }
                }
            };
            // (in the last tile a wave whose 2048 references all lie behind the store's end has zero words only:
            // nothing to count, nothing to add -- wave-uniform, and the barrier below is taken all the same)
            const bool live = tile_lo + 2048u * (uint32_t)__builtin_amdgcn_readfirstlane((int)(tid >> 6)) < a.n_refs;
            // (counts up to nd: 32 - clz(nd) bits, three of them in ones / twos / fours)
            const int bits = 32 - __builtin_clz(nd);
            if (live) switch (bits > 3 ? bits - 3 : 0) {
            case 0: dense_path(std::integral_constant<int, 0>()); break;
            case 1: dense_path(std::integral_constant<int, 1>()); break;
            case 2: dense_path(std::integral_constant<int, 2>()); break;
            case 3: dense_path(std::integral_constant<int, 3>()); break;
            case 4: dense_path(std::integral_constant<int, 4>()); break;
            case 5: dense_path(std::integral_constant<int, 5>()); break;
            case 6: dense_path(std::integral_constant<int, 6>()); break;
            default: dense_path(std::integral_constant<int, 7>()); break;
            }
            __syncthreads();
        }
