// region/tiles.h -- the LDS tile cache and the member masks: tile_slot ... flush_tiles.  Touches G_TW and g_ttag (the cache and its tags) and g_ws
// (cur_id, tm_pending, members_cached); the masks of evicted tiles are RCtx::tmask in HBM.  Restates curMap of RegionGrower (myLSD.cpp:519-520, :537, :549).
// The cache: 8x8-pixel tiles of packed pixel words, NT slots, slot = (tx + 5 ty) mod NT (rows, columns
// and diagonals of tiles spread over all slots).  RegionGrower reads its 3x3 neighbourhoods from here, so a
// batch costs LDS latency instead of dependent HBM round trips.  A cached word is the pixel's pw with the code
// replaced by two flags: bit 0 = banned (code 1 or 3), bit 1 = member of the current grow (curMap).  The member
// flags live in the cache; a tile that is evicted with members leaves them in HBM as a 64-bit mask tagged with the
// grow's id (`tmask`, 16 bytes per tile and wave), and takes them back when it returns.  (Until round 4 every accepted
// pixel was stamped in a 4-byte-per-pixel map instead: a scattered store per pixel and a fence in front of most tile
// fetches.)  The cache survives from seed to seed while no line is accepted in the image (a tile fetched before an
// accept could miss a ban that the snapshot of a later seed no longer flags).
__device__ __forceinline__ int tile_slot(int tx, int ty) { return (tx + 5 * ty) & (NT - 1); }

// Makes the tiles of every lane with need==true resident.  Returns false when two needed tiles map
// to the same slot (the caller retries with a smaller batch; a single 3x3 neighbourhood never conflicts).
// A tile's tag is (tile row << 16 | tile column).
__device__ __forceinline__ int tile_key(int tx, int ty) { return (ty << 16) | tx; }
__device__ __forceinline__ uint32_t tm_index(const RCtx& c, int key) { return 4u * (uint32_t)((key >> 16) * c.tilesX + (key & 0xffff)); }
// curMap of a pixel whose tile is NOT in the cache (the stages after RegionRadiusReducer, which empties the cache into tmask first):
// read past the L1, the reducer clears bits with atomics
__device__ __forceinline__ bool tm_member(const RCtx& c, int x, int y, uint32_t id) {
    const uint32_t* t = c.tmask + tm_index(c, tile_key(x >> 3, y >> 3));
    const int b = ((y & 7) << 3) | (x & 7);
    return __hip_atomic_load(&t[0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == id &&
           ((__hip_atomic_load(&t[2 + (b >> 5)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) >> (b & 31)) & 1u) != 0u;
}
__device__ __forceinline__ void tm_clear(const RCtx& c, int x, int y) {           // curMap(x, y) = 0
    uint32_t* t = c.tmask + tm_index(c, tile_key(x >> 3, y >> 3));
    const int b = ((y & 7) << 3) | (x & 7);
    atomicAnd(&t[2 + (b >> 5)], ~(1u << (b & 31)));
}
__device__ __forceinline__ bool ensure_tiles(const RCtx& c, bool need, int px, int py) {
    const int lane = c.lane, w = c.w, h = c.h, wave = c.wave;
    const int tx = px >> 3, ty = py >> 3;
    const int tile = need ? tile_key(tx, ty) : -1;
    const int slot = tile_slot(tx, ty);
    unsigned long long todo = ballot64(need & (g_ttag[wave][slot] != tile));
    if (!todo) return true;
    // conflict check over all needed tiles (resident ones included)
    {
        unsigned long long chk = ballot64(need);
        while (chk) {
            const int l = __builtin_ctzll(chk);
            const int T = __builtin_amdgcn_readlane(tile, l), S = __builtin_amdgcn_readlane(slot, l);
            if (ballot64(need & (slot == S) & (tile != T))) return false;
            chk &= ~ballot64(tile == T);
        }
    }
    [[maybe_unused]] const long long tt0 = NOW();
    if (__builtin_amdgcn_readfirstlane(g_ws[wave].tm_pending)) { wg_fence(); g_ws[wave].tm_pending = 0; }   // masks of tiles evicted earlier must have landed before one of them is read back
    const uint32_t id = (uint32_t)__builtin_amdgcn_readfirstlane((int)g_ws[wave].cur_id);
    AS1 const uint32_t* const pw = uglobal(c.pw);
    AS1 uint32_t* const tm = uglobal(c.tmask);
    const int lx = lane & 7, ly = lane >> 3;
    while (todo) {
        // up to 4 missing tiles per round, all loads in flight together
        int T[4], S[4];
        int nt = 0;
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            T[j] = -1; S[j] = 0;
            if (todo) {
                const int l = __builtin_ctzll(todo);
                T[j] = __builtin_amdgcn_readlane(tile, l);
                S[j] = __builtin_amdgcn_readlane(slot, l);
                todo &= ~ballot64(tile == T[j]);
                nt++;
            }
        }
        DSTAT(ST_WRING, nt);                               // (developer build: tiles fetched)
        // the tiles that make room leave their member flags in HBM (most have none: nothing is stored for them)
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j < nt) {
                const int old = __builtin_amdgcn_readfirstlane(g_ttag[wave][S[j]]);
                const unsigned long long om = old != -1 ? ballot64((G_TW(wave)[S[j] * 64 + lane] & 2u) != 0u) : 0ull;
                if (om) {
                    if (lane == 0) {
                        typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));
                        const u32x4 rec = {id, 0u, (uint32_t)om, (uint32_t)(om >> 32)};
                        *reinterpret_cast<AS1 u32x4*>(tm + tm_index(c, old)) = rec;
                    }
                    g_ws[wave].tm_pending = 1;                 // (all lanes, same value)
                }
            }
        }
        uint32_t vw[4], vi[4], vm[4];
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            vw[j] = kPwStatic; vi[j] = 0u; vm[j] = 0u;            // outside the image: banned
            if (j < nt) {
                const int x = (T[j] & 0xffff) * 8 + lx, y = (T[j] >> 16) * 8 + ly;
                if ((x < w) & (y < h)) vw[j] = pw[(uint32_t)(y * w + x)];
                AS1 const uint32_t* t = tm + tm_index(c, T[j]);
                vi[j] = t[0]; vm[j] = t[2 + (lane >> 5)];          // (two addresses per tile for the whole wave)
            }
        }
        #pragma unroll
        for (int j = 0; j < 4; j++) {
            if (j < nt) {
                const uint32_t mem = (vi[j] == id) ? ((vm[j] >> (lane & 31)) & 1u) : 0u;
                G_TW(wave)[S[j] * 64 + lane] = (vw[j] & ~3u) | (vw[j] & 1u) | (mem << 1);
                g_ttag[wave][S[j]] = T[j];                 // (all lanes, same value)
            }
        }
    }
    DSTAT(ST_TTILES, NOW() - tt0);
    return true;
}

__device__ __forceinline__ void invalidate_tiles(const RCtx& c) {
    if (c.lane < NT) g_ttag[c.wave][c.lane] = -1;
    g_ws[c.wave].members_cached = 0;
}
// Empties the cache into tmask: afterwards curMap of the current grow is in HBM in full (RegionRadiusReducer clears bits there, the
// marking stages read them there).
__device__ __forceinline__ void flush_tiles(const RCtx& c) {
    const uint32_t id = g_ws[c.wave].cur_id;
    for (int sl = 0; sl < NT; sl++) {
        const int old = __builtin_amdgcn_readfirstlane(g_ttag[c.wave][sl]);
        if (old == -1) continue;
        const unsigned long long om = ballot64((G_TW(c.wave)[sl * 64 + c.lane] & 2u) != 0u);
        if (om && c.lane == 0) {
            uint32_t* t = c.tmask + tm_index(c, old);
            t[0] = id; t[1] = 0u; t[2] = (uint32_t)om; t[3] = (uint32_t)(om >> 32);
        }
    }
    invalidate_tiles(c);
    wg_fence();
    g_ws[c.wave].tm_pending = 0;
}
