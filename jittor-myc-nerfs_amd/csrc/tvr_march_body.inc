// tvr_march_body.inc — the BODY of the march kernels, included as text inside march_kernel (tvr_march.hip) and cp_march_kernel (tvr_cp.hip); csrc/tvr_march.hip has the
// description.  Everything but the density evaluation — ray entry, sampling, in-box / alpha mask, cell indices, the transmittance scan, the queue, the dense outputs, the
// counters — is this one text, so both kernels produce the same bits for the same rays, box and grid.  (As text and not as an inlined function: the instruction stream of
// march_kernel is then what it was when the body stood in the kernel itself — a forceinline function taking the kernel's arguments compiled to 20 - 100 more instructions.)
// Expects in scope: constexpr bool DENSE, LDSL, CP, VOL; sc, rays, n_rays, S, s_cap, sm, eps_T, mo, dn (the kernel's arguments), `cp` (CpDev; unused unless CP) and
// `dvol` (the baked density volume, tvr_scene_set_density_volume; unused unless VOL).
    static_assert(!(CP && LDSL), "the CP lines (up to 96 channels) do not go through LDS");
    static_assert(!(VOL && (CP || LDSL)), "the baked volume replaces the factored evaluation: no lines in LDS, no CP lines");
    // LDS: [cursor 16 B][lines: 3 x (L+1) x 4 float4, LDSL only][per-wave weight lists f32 s_cap][per-wave sample lists u16 s_cap][MARCH_BATCH, 16-byte aligned: per-wave records of the rays that wait for their reservation]
    extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
    const int lane = threadIdx.x & 63;
    const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const int n_waves = blockDim.x >> 6;
    unsigned *cursor = (unsigned *)lds_raw;
    const float4 *ls0 = (const float4 *)(lds_raw + MARCH_HDR);
    const int ln0 = LDSL ? (sc.grid[2] + 1) * MARCH_LSTRIDE : 0, ln1 = LDSL ? (sc.grid[1] + 1) * MARCH_LSTRIDE : 0, ln2 = LDSL ? (sc.grid[0] + 1) * MARCH_LSTRIDE : 0;
    const float4 *ls1 = ls0 + ln0, *ls2 = ls1 + ln1;                     // line i runs along axis vecMode[i] = 2 - i
    float *bufw = (float *)(ls2 + ln2) + (size_t)wave * s_cap;
    unsigned short *bufj = (unsigned short *)((float *)(ls2 + ln2) + (size_t)n_waves * s_cap) + (size_t)wave * s_cap;
#ifdef TVR_MARCH_TIMELINE                               // diagnostic build (scripts/march_timeline.py): stats[32 + 8 b ..] = {start, filled, first wave end, last wave end, chunks, rays | queue reservations << 32} of group b, 100 MHz ticks
    unsigned long long tl_chunks = 0ull, tl_rays = 0ull, tl_resv = 0ull;
    if (mo.stats && threadIdx.x == 0) mo.stats[32 + 8 * blockIdx.x] = __builtin_amdgcn_s_memrealtime();
#endif
    if (threadIdx.x == 0) *cursor = 0u;
    unsigned long long *slots = (unsigned long long *)(lds_raw + 16);
    if (threadIdx.x < MARCH_SLOTS) slots[threadIdx.x] = 0ull;
    unsigned long long *gstat = (unsigned long long *)(lds_raw + 16 + 8 * MARCH_SLOTS);       // per-group sums of the three counters: ONE global atomic each per group
    if (threadIdx.x < 3) gstat[threadIdx.x] = 0ull;                           // (4096 same-address atomics per launch cost a 4096-ray call ~100 us)
    if (LDSL) {
        float4 *dst = (float4 *)(lds_raw + MARCH_HDR);
        for (int i = threadIdx.x; i < (sc.grid[2] + 1) * 4; i += blockDim.x) dst[(i >> 2) * MARCH_LSTRIDE + (i & 3)] = sc.dline[0][i];
        for (int i = threadIdx.x; i < (sc.grid[1] + 1) * 4; i += blockDim.x) dst[ln0 + (i >> 2) * MARCH_LSTRIDE + (i & 3)] = sc.dline[1][i];
        for (int i = threadIdx.x; i < (sc.grid[0] + 1) * 4; i += blockDim.x) dst[ln0 + ln1 + (i >> 2) * MARCH_LSTRIDE + (i & 3)] = sc.dline[2][i];
    }
    __syncthreads();
#ifdef TVR_MARCH_TIMELINE
    if (mo.stats && threadIdx.x == 0) mo.stats[32 + 8 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
#endif
    const int sub = lane & 3;
    // PLAIN: the four corner rows of the baked volume as wave-uniform bases (tvr_march_body.h: vol_density32); formed once per launch
    const unsigned char *vrow[4] = {nullptr, nullptr, nullptr, nullptr};
    if constexpr (PLAIN) {
        const size_t vsy = (size_t)(sc.grid[0] + 1) * 4, vsz = vsy * (size_t)(sc.grid[1] + 1);
        vrow[0] = (const unsigned char *)dvol; vrow[1] = vrow[0] + vsy; vrow[2] = vrow[0] + vsz; vrow[3] = vrow[2] + vsy;
    }
    // clock probe (stats only): shader-clock and 100 MHz reference ticks over this workgroup's lifetime
    unsigned long long clk0 = 0ull, ref0 = 0ull;
    if (march_arg_now<PLAIN>(mo.stats, offsetof(MarchVolArgs, mo.stats)) && threadIdx.x == 0) { clk0 = __builtin_amdgcn_s_memtime(); ref0 = __builtin_amdgcn_s_memrealtime(); }

    // Tiles are taken in order from ONE global counter, so the groups sweep the image together and the queue is in ~raster order (measured: march 7.9 vs 8.8 ms and
    // shade 15.25 vs 15.65 ms against per-XCD contiguous bands), and a launch with few tiles per group has no tail.
    unsigned long long st_eval = 0, st_bbox = 0, st_term = 0;
    int last_start = 0;                                  // first ray of this wave's previous handout (dynamic queue: picks the tail granularity)

    // MARCH_BATCH (tvr_march_body.h): the wave's list is a ring of s_cap entries; [ring_head, ring_head + pend_total) are the entries of the n_pend finished rays that
    // wait for their reservation, the ray in progress appends behind them.  The waiting rays' records stand behind the groups' lists in LDS.
    // The three numbers are the same in every lane and are KEPT IN VECTOR REGISTERS (the empty asm makes them opaque): the chunk loop has no scalar register to spare
    // (tvr_march_body.h, the scalar budget) and what it does with them — an entry's position, the test for room — is vector arithmetic anyway.
    int ring_head = 0, pend_total = 0, n_pend = 0;
    float *pend = nullptr;
    if constexpr (MARCH_BATCH) {
        pend = (float *)(lds_raw + ((MARCH_HDR + (size_t)n_waves * s_cap * 6 + 15) & ~(size_t)15)) + (size_t)wave * (MARCH_PEND * MARCH_PEND_WORDS);
        asm volatile("" : "+v"(ring_head), "+v"(pend_total), "+v"(n_pend));
    }

    for (;;) {
        unsigned ci = 0;
        if (lane == 0) ci = atomicAdd(cursor, 1u);
        ci = __builtin_amdgcn_readfirstlane(ci);
        // the wave that draws the first ray of local tile k takes the next global tile and publishes it {k + 1, tile} in slot k & (MARCH_SLOTS - 1); the others
        // wait for the slot's generation to become k + 1.  Why the wait ends: the publisher stores right behind its draw (one global atomic,
        // ~2 us), and the slot is only overwritten by the publisher of local tile k + 64, which needs the group's cursor to advance by 1024 draws
        // and 64 later publishers to have finished their own global atomic first.  The wait is nevertheless BOUNDED and a miss is LOUD:
        // a waiter that finds a later generation in its slot (it was overtaken) or spins MARCH_SPIN_LIMIT times raises mo.counter[2], stops
        // drawing rays, and the composite kernel then writes NaN to every pixel of the call (tvr.h: tvr_scratch_layout.counter).
        // Round 3: the counter counts RAYS, and a handout is 16 rays (a tile: concurrent neighbours share texels in L1) until the launch's last
        // 2 x 16 x groups rays, which go out 4 at a time: the groups then end within one ray of each other instead of two (a group that draws a
        // whole tile just before the counter runs out works 2 x 60 us after everybody else stopped drawing).  Measured on rank 0's share of an 8-way
        // split (81 920 rays, interleaved A/B on one box): 1.03 - 1.06 ms against 1.06 - 1.07 — about 1 %; the rest of that share's loss against 1/8
        // of a frame (0.98 ms) is the ramp at both ends of a launch whose unit of work is a whole ray.  Local tiles keep 16 cursor positions;
        // positions >= the handout's length are no-ops.
        int ray_start, ray_len;
        {
            const unsigned k = ci / MARCH_TILE, slot = k & (MARCH_SLOTS - 1u);
            if ((ci % MARCH_TILE) == 0u) {
                unsigned t = 0, len = MARCH_TILE;
                if (lane == 0) {
                    // how far the launch is: the first ray of THIS wave's previous handout (a register; one ray-time stale, the tail zone is two tiles per
                    // group wide).  Not a fresh look at the counter: an agent-scope load of that line between the atomics of 4096 waves cost the kernel
                    // 30 % (10.1 vs 7.7 ms: every system-coherent read forces the line the queue-length atomics hammer out of L2).
                    // (launches of fewer than 8 tiles per group keep whole tiles: there the 16 concurrent neighbours' shared texels matter more than the tail)
                    if ((long long)n_rays >= 8LL * MARCH_TILE * (long long)gridDim.x && (long long)last_start + 2LL * MARCH_TILE * (long long)gridDim.x >= (long long)n_rays)
                        len = MARCH_TAIL;
                    t = atomicAdd(march_arg_now<PLAIN>(mo.counter, offsetof(MarchVolArgs, mo.counter)) + MARCH_CTR_WORD, len);
                    const unsigned long long genw = (unsigned long long)(k + 1u) | (len == MARCH_TAIL ? 0x80000000ull : 0ull);
#ifdef TVR_FAULT_INJECT_MARCH                          // test build only (tests/test_gpu_faults.py): the publisher of local tile 3 of group 0 skips a generation
                    if (blockIdx.x == 0 && k == 3u) __hip_atomic_store(&slots[slot], ((unsigned long long)(k + 1u + MARCH_SLOTS) << 32) | t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    else
#endif
                    __hip_atomic_store(&slots[slot], (genw << 32) | t, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_WORKGROUP);
                }
                ray_start = (int)__builtin_amdgcn_readfirstlane(t);
                ray_len = (int)__builtin_amdgcn_readfirstlane(len);
            } else {
                unsigned long long v;
                unsigned spins = 0u, fault = 0u;
                for (;;) {
                    v = __hip_atomic_load(&slots[slot], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_WORKGROUP);
                    const unsigned gen = (unsigned)(v >> 32) & 0x7fffffffu;
                    if (gen == k + 1u) break;
                    if (gen > k + 1u) { fault = 1u; break; }                       // overtaken: this tile's number is gone
                    if (++spins > MARCH_SPIN_LIMIT) { fault = 2u; break; }         // the publisher never stored
                    __builtin_amdgcn_s_sleep(1);
                }
                if (fault) {
                    if (lane == 0) atomicOr(march_arg_now<PLAIN>(mo.counter, offsetof(MarchVolArgs, mo.counter)) + 2, fault);
                    break;
                }
                ray_start = (int)(unsigned)v;
                ray_len = (v >> 63) ? MARCH_TAIL : MARCH_TILE;
            }
        }
        if (ray_start >= n_rays) break;
        if ((int)(ci % MARCH_TILE) >= ray_len) continue;
        last_start = ray_start;
        const int ray = ray_start + (int)(ci % MARCH_TILE);
        if (ray >= n_rays) continue;
        // (PLAIN reads what it needs once per ray from the kernel-argument segment, here and behind the chunk loop: tvr_march_body.h, march_arg_now)
        const float *__restrict__ const rays_r = march_arg_now<PLAIN>(rays, offsetof(MarchVolArgs, rays));
        const float *const jit_r = march_arg_now<PLAIN>(sm.jitter, offsetof(MarchVolArgs, sm.jitter));
        float o[3], d[3];
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            o[k] = rays_r[(size_t)ray * 6 + k];
            d[k] = rays_r[(size_t)ray * 6 + 3 + k];
        }
        const float tmin = ray_tmin(sc, o, d);
        const bool has_jit = jit_r != nullptr;
        const float u = has_jit ? jit_r[ray] : 0.0f;
        const float *__restrict__ zrow = (!PLAIN && sm.zv) ? sm.zv + (size_t)ray * S : nullptr;     // explicit depths (wave-uniform choice)
        float lam6 = 1.0f;
        int n6 = 0;                                        // samples whose (1 - alpha + 1e-6) factor lam6 already holds

        float T = 1.0f, acc_l = 0.0f, dep_l = 0.0f;
        int napp = 0;
        bool seen = false, terminated = false;
        int c = 0;
        bool make_room = false;                            // MARCH_BATCH: the chunk loop was left for a flush and goes on at chunk c
        for (;;) {
        for (; c * 64 < S; ++c) {
            if constexpr (MARCH_BATCH) {
                // Before a chunk, never inside one (the flush's registers would be the chunk loop's): the waiting rays leave when MARCH_PEND of them wait or when
                // they hold room this chunk's up to 64 entries may need.  A ray alone never exceeds s_cap, so behind the flush the chunk always fits.
                if (__ballot(n_pend > 0 && (n_pend == MARCH_PEND || pend_total + napp + 64 > s_cap))) { make_room = true; break; }      // (the ballot: a scalar branch)
            }
            const int j = c * 64 + lane;
            const bool inr = j < S;
            float fj = (float)j, fj1 = (float)(j + 1);
            if (has_jit) { fj = fj + u; fj1 = fj1 + u; }
            float z = tmin + sc.step * fj;                     // tensorBase.py:354-355
            float z1 = tmin + sc.step * fj1;
            if (zrow) {
                z = inr ? zrow[j] : 0.0f;
                z1 = (j < S - 1) ? zrow[j + 1] : z;
            }
            float p[3], n[3], f[3];
            bool bbox = inr;
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                p[k] = o[k] + d[k] * z;                        // :357
                bbox = bbox & !((sc.lo[k] > p[k]) | (p[k] > sc.hi[k]));   // :358
            }
            bool valid = bbox;
            if (!PLAIN && sc.avol != nullptr) {
                if (bbox) valid = sc.abits ? alpha_positive(sc, p) : (alpha_lookup(sc, p) > 0.0f);  // :491-496
            }
            int i0[3];
            float w[3];
#pragma unroll
            for (int k = 0; k < 3; ++k) {
                n[k] = (p[k] - sc.lo[k]) * sc.inv[k] - 1.0f;   // :223-224
                f[k] = unnorm(n[k], sc.gm1[k]);
                const float fl = floorf(f[k]);
                i0[k] = (int)fl;
                w[k] = f[k] - fl;
            }
            if constexpr (PLAIN) asm volatile("" : "+v"(i0[0]), "+v"(i0[1]), "+v"(i0[2]), "+v"(w[0]), "+v"(w[1]), "+v"(w[2]));   // one computation per sample: not rematerialised in the valid branch
            const unsigned long long mb = __ballot(bbox), mv = __ballot(valid);
            if (DENSE) {
                const size_t q = (size_t)ray * S + j;
                if (inr) {
                    if (dn.z) dn.z[q] = z;
                    if (dn.valid) dn.valid[q] = valid;
                    if (dn.bbox_valid) dn.bbox_valid[q] = bbox;
                    if (dn.cell) { dn.cell[q * 3] = i0[0]; dn.cell[q * 3 + 1] = i0[1]; dn.cell[q * 3 + 2] = i0[2]; }
                }
            }
            st_bbox += __popcll(mb);
            if (mv == 0ull) {
                // no density anywhere in this chunk: alpha = 0, T unchanged (1 - 0 + 1e-10 == 1 in fp32), weights 0
                if (DENSE && inr) {
                    const size_t q = (size_t)ray * S + j;
                    if (dn.sigma_feature) dn.sigma_feature[q] = 0.f;
                    if (dn.sigma) dn.sigma[q] = 0.f;
                    if (dn.alpha) dn.alpha[q] = 0.f;
                    if (dn.weight) dn.weight[q] = 0.f;
                }
                if (mb == 0ull && seen && !DENSE) break;        // left the (convex) box: nothing further can be valid
                continue;
            }
            seen = true;
            st_eval += __popcll(mv);
#ifdef TVR_MARCH_TIMELINE
            tl_chunks++;
#endif

            // ---- density feature ----
            float sf = 0.0f;
            if constexpr (VOL) {
                // baked volume (tvr_march_body.h: vol_density): lane per sample, the trilinear interpolation of the cell's eight corner values
                if constexpr (PLAIN) {
                    if (valid) sf = vol_density32(vrow[0], vrow[1], vrow[2], vrow[3], (unsigned)(sc.grid[0] + 1), (unsigned)(sc.grid[1] + 1), i0[0], i0[1], i0[2], w[0], w[1], w[2]);
                } else
                if (valid) sf = vol_density(dvol, sc.grid[0] + 1, sc.grid[1] + 1, i0[0], i0[1], i0[2], w[0], w[1], w[2]);
            } else {
                // factored form: 4 sub-steps, quad-per-sample gather
#pragma unroll
                for (int k4 = 0; k4 < 4; ++k4) {
                    const bool v = quad_bcast_i((int)valid, k4) != 0;
                    if (__ballot(v) == 0ull) continue;
                    const int ix = quad_bcast_i(i0[0], k4), iy = quad_bcast_i(i0[1], k4), iz = quad_bcast_i(i0[2], k4);
                    const float wx = quad_bcast_f(w[0], k4), wy = quad_bcast_f(w[1], k4), wz = quad_bcast_f(w[2], k4);
                    float part = 0.0f;
                    if constexpr (CP) {
                        if (v) part = cp_density_quad(sc, cp, ix, iy, iz, wx, wy, wz, sub);
                    } else
                    if (v && LDSL) {
                        const float4 a = vm_term_lds(sc.dplane[0], ls0, sc.grid[0], ix, iy, iz, wx, wy, wz, sub);
                        const float4 b = vm_term_lds(sc.dplane[1], ls1, sc.grid[0], ix, iz, iy, wx, wz, wy, sub);
                        const float4 cc = vm_term_lds(sc.dplane[2], ls2, sc.grid[1], iy, iz, ix, wy, wz, wx, sub);
                        part = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((cc.x + cc.y) + (cc.z + cc.w));
                    } else if (v) {
                        // plane0 (x,y)·line0(z) ; plane1 (x,z)·line1(y) ; plane2 (y,z)·line2(x)   (matMode / vecMode)
                        const float4 a = vm_term<4, false>(sc.dplane[0], sc.dline[0], sc.grid[0], sc.grid[1], sc.grid[2], ix, iy, iz, wx, wy, wz, sub);
                        const float4 b = vm_term<4, false>(sc.dplane[1], sc.dline[1], sc.grid[0], sc.grid[2], sc.grid[1], ix, iz, iy, wx, wz, wy, sub);
                        const float4 cc = vm_term<4, false>(sc.dplane[2], sc.dline[2], sc.grid[1], sc.grid[2], sc.grid[0], iy, iz, ix, wy, wz, wx, sub);
                        part = ((a.x + a.y) + (a.z + a.w)) + ((b.x + b.y) + (b.z + b.w)) + ((cc.x + cc.y) + (cc.z + cc.w));
                    }
                    part += quad_perm_f<QUAD_XOR1>(part);
                    part += quad_perm_f<QUAD_XOR2>(part);
                    if (sub == k4) sf = part;
                }
            }

            float sigma = 0.0f;
            constexpr bool LEAN = VOL && MARCH_VOL_LEAN;          // the volume marches' own exp / softplus (tvr_march_body.h)
            if constexpr (LEAN) {
                if (valid) sigma = (sc.act == 0) ? march_softplus(sf + sc.shift) : fmaxf(sf, 0.0f);
            } else
            if (valid) sigma = (sc.act == 0) ? softplus_f(sf + sc.shift) : fmaxf(sf, 0.0f);   // :444-448
            float dist = (j < S - 1) ? (z1 - z) : 0.0f;           // :488
            dist = dist * sc.scale;                               // :511
            const float alpha = 1.0f - (LEAN ? march_expf(-sigma * dist) : expf(-sigma * dist));       // :19
            const float fT = (1.0f - alpha) + 1e-10f;             // :21
            if (!PLAIN && mo.lam6) {                              // nerfplusplus.py:277: cumprod(1 - alpha + TINY_NUMBER), TINY_NUMBER = 1e-6
                float f6 = inr ? (1.0f - alpha) + 1e-6f : 1.0f;
#pragma unroll
                for (int off = 32; off > 0; off >>= 1) f6 = f6 * __shfl_xor(f6, off);
                lam6 = lam6 * f6;
                n6 += min(64, S - c * 64);
            }
            float incl = fT, excl, last;
            if constexpr (VOL) {
                scan_mul_dpp(incl, excl, last);                    // the same products in the same order, moved by DPP / permlane swaps instead of through LDS
            } else {
#pragma unroll
                for (int off = 1; off < 64; off <<= 1) {
                    const float t = __shfl_up(incl, off);
                    if (lane >= off) incl = incl * t;
                }
                excl = __shfl_up(incl, 1);
                if (lane == 0) excl = 1.0f;
            }
            const float Tj = T * excl;
            const float wgt = alpha * Tj;                          // :23
            acc_l += wgt;
            dep_l += wgt * z;
            const bool app = wgt > sc.thres;                       // :513
            const unsigned long long ma = __ballot(app);
            if constexpr (MARCH_BATCH) {
                if (ma) {
                    int pos = ring_head + pend_total + napp + __popcll(ma & ((1ull << lane) - 1ull));
                    if (pos >= s_cap) pos -= s_cap;
                    if (app) { bufw[pos] = wgt; bufj[pos] = (unsigned short)j; }
                    napp += __popcll(ma);
                }
            } else
            if (ma) {
                const int pos = napp + __popcll(ma & ((1ull << lane) - 1ull));
                if (app) { bufw[pos] = wgt; bufj[pos] = (unsigned short)j; }
                napp += __popcll(ma);
            }
            if constexpr (VOL) T = T * last;
            else T = T * __shfl(incl, 63);
            if (DENSE && inr) {
                const size_t q = (size_t)ray * S + j;
                if (dn.sigma_feature) dn.sigma_feature[q] = valid ? sf : 0.f;
                if (dn.sigma) dn.sigma[q] = sigma;
                if (dn.alpha) dn.alpha[q] = alpha;
                if (dn.weight) dn.weight[q] = wgt;
            }
            if (T < eps_T) { terminated = true; ++c; break; }
        }
        if (!make_room) break;
#ifdef TVR_MARCH_TIMELINE
        tl_resv++;
#endif
        if constexpr (MARCH_BATCH) march_flush<PLAIN>(sc, sm, mo, S, s_cap, lane, bufw, bufj, pend, ring_head, pend_total, n_pend);
        make_room = false;
        }
        if (DENSE) {
            // samples never visited (early exit) get zeros so the dense arrays are fully defined
            for (int cc = c; cc * 64 < S; ++cc) {
                const int j = cc * 64 + lane;
                if (j < S) {
                    const size_t q = (size_t)ray * S + j;
                    const float fjj = has_jit ? ((float)j + u) : (float)j;
                    if (dn.z) dn.z[q] = zrow ? zrow[j] : tmin + sc.step * fjj;
                    if (dn.valid) dn.valid[q] = 0;
                    if (dn.bbox_valid) dn.bbox_valid[q] = 0;
                    if (dn.cell) { dn.cell[q * 3] = 0; dn.cell[q * 3 + 1] = 0; dn.cell[q * 3 + 2] = 0; }
                    if (dn.sigma_feature) dn.sigma_feature[q] = 0.f;
                    if (dn.sigma) dn.sigma[q] = 0.f;
                    if (dn.alpha) dn.alpha[q] = 0.f;
                    if (dn.weight) dn.weight[q] = 0.f;
                }
            }
        }
        st_term += terminated ? 1 : 0;
#ifdef TVR_MARCH_TIMELINE
        tl_rays++;
#endif

        const float acc = wave_sum(acc_l);
        const float dep = wave_sum(dep_l);
        const MarchOut mt = march_arg_now<PLAIN>(mo, offsetof(MarchVolArgs, mo));
        if constexpr (MARCH_BATCH) {
            // the ray's own outputs now; its entries and ray_off with the wave's next reservation (march_flush)
            if (lane == 0) {
                if (napp == 0) mt.ray_off[ray] = 0u;
                mt.ray_cnt[ray] = (unsigned)napp;
                mt.acc[ray] = acc;
                mt.depth[ray] = dep + (1.0f - acc) * d[2];            // :531 (rays[..., -1] is d_z)
                if (!PLAIN && mt.lam6) mt.lam6[ray] = lam6 * expf((float)(S - n6) * 9.5367386e-7f);
                if (DENSE) {
                    if (dn.bg_weight) dn.bg_weight[ray] = T;
                    if (dn.acc) dn.acc[ray] = acc;
                    if (dn.t_min) dn.t_min[ray] = tmin;
                }
            }
            if (napp > 0) {
                if (lane == 0) {
                    float *rec = pend + n_pend * MARCH_PEND_WORDS;      // (n_pend < MARCH_PEND: a full set left before this ray's first chunk)
                    rec[0] = o[0]; rec[1] = o[1]; rec[2] = o[2];
                    rec[3] = d[0]; rec[4] = d[1]; rec[5] = d[2];
                    rec[6] = tmin; rec[7] = u;
                    rec[8] = __uint_as_float((unsigned)ray); rec[9] = __uint_as_float((unsigned)pend_total);
                }
                pend_total += napp;
                ++n_pend;
                asm volatile("" : "+v"(pend_total), "+v"(n_pend));
            }
            continue;
        }
        unsigned base = 0;
#ifdef TVR_MARCH_TIMELINE
        if (napp > 0) tl_resv++;
#endif
        if (lane == 0 && napp > 0) base = atomicAdd(mt.counter, (unsigned)napp);
        base = __shfl(base, 0);
        if (lane == 0) {
            mt.ray_off[ray] = base;
            mt.ray_cnt[ray] = (unsigned)napp;
            mt.acc[ray] = acc;
            mt.depth[ray] = dep + (1.0f - acc) * d[2];            // :531 (rays[..., -1] is d_z)
            // samples of skipped chunks / behind an early exit have alpha = 0: each factor is fp32(1 + 1e-6) = 1 + 8 ulp, log = 9.5367386e-7
            if (!PLAIN && mt.lam6) mt.lam6[ray] = lam6 * expf((float)(S - n6) * 9.5367386e-7f);
            if (DENSE) {
                if (dn.bg_weight) dn.bg_weight[ray] = T;
                if (dn.acc) dn.acc[ray] = acc;
                if (dn.t_min) dn.t_min[ray] = tmin;
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        for (int i = lane; i < napp; i += 64) {
            const unsigned ej = bufj[i];
            float fj = (float)ej;
            if (has_jit) fj = fj + u;
            const float z = zrow ? zrow[ej] : tmin + sc.step * fj;
            float4 qv;
            qv.x = ((o[0] + d[0] * z) - sc.lo[0]) * sc.inv[0] - 1.0f;
            qv.y = ((o[1] + d[1] * z) - sc.lo[1]) * sc.inv[1] - 1.0f;
            qv.z = ((o[2] + d[2] * z) - sc.lo[2]) * sc.inv[2] - 1.0f;
            qv.w = bufw[i];
            mt.q_pos[base + i] = qv;
            mt.q_ray[base + i] = (unsigned)ray;
            if (mt.q_j) mt.q_j[base + i] = ej;
        }
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    }
    if constexpr (MARCH_BATCH) {
#ifdef TVR_MARCH_TIMELINE
        if (__ballot(n_pend > 0)) tl_resv++;
#endif
        if (__ballot(n_pend > 0)) march_flush<PLAIN>(sc, sm, mo, S, s_cap, lane, bufw, bufj, pend, ring_head, pend_total, n_pend);       // every exit of the ray loop comes through here: the queue ran out, or one of the two fault breaks
    }
#ifdef TVR_MARCH_TIMELINE
    if (mo.stats && lane == 0) {
        const unsigned long long te = __builtin_amdgcn_s_memrealtime();
        atomicMin((unsigned long long *)&mo.stats[32 + 8 * blockIdx.x + 2], te);
        atomicMax((unsigned long long *)&mo.stats[32 + 8 * blockIdx.x + 3], te);
        atomicAdd((unsigned long long *)&mo.stats[32 + 8 * blockIdx.x + 4], tl_chunks);
        atomicAdd((unsigned long long *)&mo.stats[32 + 8 * blockIdx.x + 5], tl_rays | (tl_resv << 32));
    }
#endif
    unsigned long long *const stats_r = march_arg_now<PLAIN>(mo.stats, offsetof(MarchVolArgs, mo.stats));
    if (stats_r) {                                       // (wave-uniform: every wave of the group reaches this barrier exactly once)
        if (lane == 0) {
            atomicAdd(&gstat[0], st_eval);
            atomicAdd(&gstat[1], st_bbox);
            atomicAdd(&gstat[2], st_term);
        }
        __syncthreads();
        if (threadIdx.x == 0) {
            atomicAdd((unsigned long long *)&stats_r[TVR_STAT_SAMPLES_EVAL], gstat[0]);
            atomicAdd((unsigned long long *)&stats_r[TVR_STAT_SAMPLES_BBOX], gstat[1]);
            atomicAdd((unsigned long long *)&stats_r[TVR_STAT_RAYS_TERMINATED], gstat[2]);
            atomicAdd((unsigned long long *)&stats_r[TVR_STAT_MARCH_CLK], __builtin_amdgcn_s_memtime() - clk0);
            atomicAdd((unsigned long long *)&stats_r[TVR_STAT_MARCH_REF], __builtin_amdgcn_s_memrealtime() - ref0);
        }
    }
