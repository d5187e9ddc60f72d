// lstm_fwd_bf_step.inc -- ONE time step of lstm_fwd_bf_body (lstm_persistent.hip), included as the body of its time loop: once for the
// plain kernel's loop over all T steps, once for the guarded kernel's loop over a segment of them.  Two copies of the same text, so
// that the plain instantiations compile to what they were before the guarded ones existed (registers pinned by
// tests/test_kernel_resources.py and tests/golden/plans.json).  Uses the enclosing function's locals; `step` is the loop variable.
    const int t = dir == 0 ? step : T - 1 - step;
    const int tp = dir == 0 ? t - 1 : t + 1;
    f32x4 acc[NT];
#pragma unroll
    for (int n = 0; n < NT; ++n) acc[n] = f32x4{0.f, 0.f, 0.f, 0.f};
    EESEN_STAMP(0);
    if (step > 0) {
      if (wave == EESEN_POLL_WAVE) {
        const bool go = wait_counters(my_cnt, nblk, (unsigned)step, err, spin_limit, lane, L.poll_delay);
        if (lane == 0) s_go = go ? 1 : 0;
      }
      __syncthreads();
      if (!s_go) return;
      EESEN_STAMP(1);
      if (L.milestone && step == L.milestone_step + 1 && bx == 0 && tid == 0)
        report_milestone(L.milestone, (unsigned)(R.ndir * R.nz));
      const unsigned xb = ((unsigned)(tp * L.ndir + dir) * (unsigned)nzall + (unsigned)zt) * xblk;
      constexpr unsigned kOob = 0x80000000u;
      const bool rok = s0 + li < s_end;
      f32x4 a[AP][CPW];
#pragma unroll
      for (int pl = 0; pl < AP; ++pl)
#pragma unroll
        for (int c = 0; c < CPW; ++c) {
          const int ch = wave + c * NW;
          a[pl][c] = __builtin_amdgcn_raw_buffer_load_b128(rX, (rok && ch < nch) ? xb + (unsigned)pl * xpl + (unsigned)(((ch * 4 + kq) * 16 + li) * 16) : kOob, 0, 0);
        }
      __builtin_amdgcn_sched_barrier(0);
#pragma unroll
      for (int sum = SMAX; sum >= 0; --sum)      // the smallest cross products first
#pragma unroll
        for (int i = 0; i < AP; ++i) {
          const int j = sum - i;
          if (j < 0 || j >= WP) continue;
#pragma unroll
          for (int c = 0; c < CPW; ++c)
#pragma unroll
            for (int n = 0; n < NT; ++n) {
              const f32x4& bb = b[j < WP && j >= 0 ? j : 0][n][c];
              if constexpr (F16) acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_f16(__builtin_bit_cast(f16x8_t, a[i][c]), __builtin_bit_cast(f16x8_t, bb), acc[n], 0, 0, 0);
              else acc[n] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(__builtin_bit_cast(bf16x8_t, a[i][c]), __builtin_bit_cast(bf16x8_t, bb), acc[n], 0, 0, 0);
            }
        }
    }
#pragma unroll
    for (int n = 0; n < NT; ++n)
#pragma unroll
      for (int r = 0; r < 4; ++r) red[wave][4 * kq + r][n * 16 + li] = F16 ? acc[n][r] * unscale : acc[n][r];
    __syncthreads();
    EESEN_STAMP(2);
    if (e_act) {
      // the eight waves' partial sums: ALL eight LDS reads in flight, then the sum in the same order (hipcc kept two in flight and
      // waited for each in turn: eight ~100-cycle round trips on the step's critical path)
      float4 pv[NW];
#pragma unroll
      for (int w = 0; w < NW; ++w) pv[w] = *reinterpret_cast<const float4*>(&red[w][es][eu * 4]);
      __builtin_amdgcn_sched_barrier(0);
      float4 pre = gx;
#pragma unroll
      for (int w = 0; w < NW; ++w) { pre.x += pv[w].x; pre.y += pv[w].y; pre.z += pv[w].z; pre.w += pv[w].w; }
      float g = tanhf_(pre.x);
      float i = sigmoidf_(pre.y + p_i * cprev);
      float f = sigmoidf_(pre.z + p_f * cprev);
      float c = g * i + cprev * f;
      float h = tanhf_(c);
      float o = sigmoidf_(pre.w + p_o * c);
      float m = h * o;
      if (t >= len || !e_ok) { g = i = f = o = c = m = 0.f; }
      if (e_ok) {
        *reinterpret_cast<float4*>(L.G + (size_t)(t * S + s_e) * ldG + gcol) = make_float4(g, i, f, o);
        const size_t o1 = (size_t)((t + 1) * S + s_e) * ldY + dir * H + u0 + eu;
        L.C[o1] = c;
        __hip_atomic_store(L.Y + o1, m, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        cprev = c;
      }
      // the AP planes of m: four adjacent units -> one 8-byte word per plane (a single 8-byte store is single-copy atomic; write-through)
      const int k = u0 + eu;
      const size_t xo = ((size_t)(t * L.ndir + dir) * nzall + zt) * (size_t)xblk +
                        (size_t)((((k >> 5) * 4 + ((k & 31) >> 3)) * 16 + es) * 16 + (k & 7) * 2);
      float rem = F16 ? m * kMScale : m;
#pragma unroll
      for (int pl = 0; pl < AP; ++pl) {
        const unsigned hb = F16 ? rne_f16(rem) : rne_bf16(rem);
        rem -= F16 ? f16_bits_to_f32(hb) : __uint_as_float(hb << 16);          // exact
        const unsigned pk = hb | (quad_xor1(hb) << 16);                        // valid in even lanes: (unit eu, eu + 1)
        const unsigned pk2 = quad_xor2(pk);                                     // lanes eu % 4 == 0: the pair of (eu + 2, eu + 3)
        if (e_ok && (eu & 3) == 0)
          __hip_atomic_store(reinterpret_cast<unsigned long long*>(xbytes + xo + (size_t)pl * xpl), (unsigned long long)pk | ((unsigned long long)pk2 << 32),
                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      }
    }
    EESEN_STAMP(3);
    {
      if (e_act) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      EESEN_STAMP(4);
      if (tid == 0) __hip_atomic_fetch_add(my_cnt + (bx & (kShards - 1)) * kShardStride, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      if (e_ok && step + 1 < T)
        gx = *reinterpret_cast<const float4*>(L.G + (size_t)((dir == 0 ? t + 1 : t - 1) * S + s_e) * ldG + gcol);
    }
