// superplus_amd/csrc/dfk_graph.inc -- SURVEY 8(f)-1 (included by dfk.hip): unipath edges on the device dictionary, the
// canonical HyperBasevector on the host, and the graph files of a.<K>/.
//
// Reference being replaced (lib/assembly/src):
//   buildEdges            paths/long/BuildReadQGraph48.cc:505-530 (EdgeBuilder :320-503)   -> k_graph_* (dfk_graph_kernels.h)
//   buildHBVFromEdges     paths/long/HBVFromEdges.cc:244-296 (vertex dictionary :132-168, canonical edge order
//                         :106-111,275-277, HBVBuilder's queue-ordered numbering :170-238)  -> build_hbv() below, host
//   HyperBasevector::Involution, writeBinary; HyperBasevectorX    paths/HyperBasevector.cc:121-137,668-680
//   WriteAssemblyFiles    10X/WriteFiles.cc:69-101: a.k, a.hbv, a.to_left, a.to_right, a.inv, a.hbx, a.fastb, a.kmers
// The edge walk is pointer chasing over 3x10^9 k-mers and runs on the GPU; the numbering of vertices and edges is a
// breadth-first traversal whose order IS the result (edge ids are assigned in queue order), so it is sequential in
// the reference and sequential here, on the host, over the ~10^2 times fewer edges.
#include "dfk_graph_kernels.h"
#include "dfk_paths_kernels.h"                                       // (k_filter_build: the pather's filter is made under the numbering)

#include <array>

namespace {

struct GraphEdge { uint32_t n; uint64_t byte_off; };                 // canonical edge: k-mers, where its bases start in `bases`

struct HostGraph {
    uint32_t K = 0;
    std::vector<GraphEdge> ce;                                       // canonical edges, in the order the device found them
    std::vector<uint8_t> bases;                                      // their 2-bit bases, byte aligned per edge, LSB-first
    // the HyperBasevector
    uint64_t n_vertices = 0;
    struct HEdge { uint32_t ce; uint8_t rc; int32_t v, w; };         // HBV edge = canonical edge in one orientation, v -> w
    std::vector<HEdge> he;
    std::vector<int32_t> fwd, rev;                                   // canonical edge -> HBV edge (HBVFromEdges' translation tables)
    // digraphE's adjacency in the order AddEdge keeps it (DigraphTemplate.h:2058-2068: by neighbouring vertex, equal neighbours
    // in the order they were added), row v = [start[v], start[v + 1])
    std::vector<uint32_t> from_start, to_start;
    std::vector<int32_t> from_v, from_e, to_v, to_e;
    bool built = false;
    // what stays on the device for read pathing (row f-2): the k-mer index, the canonical edges' records and bases
    DevBuf d_index, d_recs, d_store; uint64_t index_slots = 0;
    DevBuf d_filter; uint64_t filter_words = 0;                      // the filter in front of the index (dfk_paths_kernels.h), when there was room for it
    struct PathState* paths = nullptr;                               // dfk_paths.inc
    struct PathState* hops_arrays = nullptr;                         // dfk_hops_build_arrays' result, nothing else in it (dfk_hops.inc)
    void (*paths_free)(struct PathState*) = nullptr;
    struct SubsetResult* subset_arrays = nullptr;                    // dfk_subset_build_arrays' result (dfk_subset.inc)
    void (*subset_free)(struct SubsetResult*) = nullptr;
    struct CloserResult* closer_arrays = nullptr;                    // dfk_closer_build_arrays' result (dfk_closer.inc)
    void (*closer_free)(struct CloserResult*) = nullptr;
    struct PartnersResult* partners_arrays = nullptr;                // dfk_partners_build_arrays' result (dfk_partners.inc)
    void (*partners_free)(struct PartnersResult*) = nullptr;
    struct ConsResult* cons_arrays = nullptr;                        // dfk_cons_build_arrays' result (dfk_cons.inc)
    void (*cons_free)(struct ConsResult*) = nullptr;
    struct OffsetsResult* offsets = nullptr;                         // the latest dfk_offsets_build*'s result (dfk_offsets.inc)
    void (*offsets_free)(struct OffsetsResult*) = nullptr;
    struct ClosuresResult* closures = nullptr;                       // the latest dfk_closures_build*'s result (dfk_closures.inc)
    void (*closures_free)(struct ClosuresResult*) = nullptr;
    struct WalksResult* walks = nullptr;                             // the latest dfk_walks_build*'s result (dfk_walks.inc)
    void (*walks_free)(struct WalksResult*) = nullptr;
    struct SconsResult* scons = nullptr;                             // the latest dfk_scons_build*'s result (dfk_scons.inc)
    void (*scons_free)(struct SconsResult*) = nullptr;
    struct SoffsetsResult* soffsets = nullptr;                       // the latest dfk_soffsets_build*'s result (dfk_soffsets.inc)
    void (*soffsets_free)(struct SoffsetsResult*) = nullptr;
    struct SclosuresResult* sclosures = nullptr;                     // the latest dfk_sclosures_build*'s result (dfk_sclosures.inc)
    void (*sclosures_free)(struct SclosuresResult*) = nullptr;
    struct PatchResult* patch = nullptr;                             // the latest dfk_patch_build*'s result (dfk_patch.inc)
    void (*patch_free)(struct PatchResult*) = nullptr;
    ~HostGraph()
    {
        if (paths && paths_free) paths_free(paths);
        if (hops_arrays && paths_free) paths_free(hops_arrays);
        if (subset_arrays && subset_free) subset_free(subset_arrays);
        if (closer_arrays && closer_free) closer_free(closer_arrays);
        if (partners_arrays && partners_free) partners_free(partners_arrays);
        if (cons_arrays && cons_free) cons_free(cons_arrays);
        if (offsets && offsets_free) offsets_free(offsets);
        if (closures && closures_free) closures_free(closures);
        if (walks && walks_free) walks_free(walks);
        if (scons && scons_free) scons_free(scons);
        if (soffsets && soffsets_free) soffsets_free(soffsets);
        if (sclosures && sclosures_free) sclosures_free(sclosures);
        if (patch && patch_free) patch_free(patch);
    }
};

inline uint32_t base_at(const uint8_t* p, uint64_t i) { return (p[i >> 2] >> (2 * (i & 3))) & 3u; }

// base i of HBV edge sequence (canonical edge read forward, or its reverse complement)
struct SeqView {
    const uint8_t* p; uint32_t L; bool rc;
    uint32_t operator[](uint32_t i) const { return rc ? 3u - base_at(p, L - 1 - i) : base_at(p, i); }
};

// The (K-1)-mer at base `pos` of a packed sequence as one number, base 0 lowest (K-1 <= 59 bases: 118 bits), and its reverse
// complement: the key of a vertex.
typedef unsigned __int128 u128h;
inline u128h kmer_at(const uint8_t* p, uint64_t n_bytes, uint64_t pos, uint32_t k)
{
    // up to 17 bytes hold it; the tail of the store may be shorter than that
    const uint64_t b0 = pos >> 2;
    uint8_t buf[24] = {0};
    memcpy(buf, p + b0, std::min<uint64_t>(17, n_bytes - b0));
    u128h x; memcpy(&x, buf, 16);
    const unsigned sh = 2 * (unsigned)(pos & 3);
    if (sh) x = (x >> sh) | ((u128h)buf[16] << (128 - sh));
    return x & ((((u128h)1) << (2 * k)) - 1);
}
inline uint64_t rev2(uint64_t x)                                    // the 32 two-bit fields of x in reverse order
{
    x = ((x >> 2) & 0x3333333333333333ull) | ((x & 0x3333333333333333ull) << 2);
    x = ((x >> 4) & 0x0F0F0F0F0F0F0F0Full) | ((x & 0x0F0F0F0F0F0F0F0Full) << 4);
    return __builtin_bswap64(x);
}
inline u128h kmer_rc_h(u128h x, uint32_t k)
{
    const u128h c = ~x;
    const u128h r = ((u128h)rev2((uint64_t)c) << 64) | rev2((uint64_t)(c >> 64));   // all 64 fields reversed: ours are the top k
    return r >> (128 - 2 * k);
}
struct VKey { uint64_t a, b; bool operator==(const VKey& o) const { return a == o.a && b == o.b; } };
inline VKey vkey_of(u128h x) { return VKey{(uint64_t)x, (uint64_t)(x >> 64)}; }
inline uint64_t vkey_hash(const VKey& k) { uint64_t h = k.a * 0x9E3779B97F4A7C15ull ^ (k.b + 0x7F4A7C159E3779B9ull) * 0xC2B2AE3D27D4EB4Full; return h ^ (h >> 29); }

// digraphE::AddEdge keeps from[v] sorted by the vertex it leads to, an equal one behind those already there: (w, edge
// number) ascending.  Rows by counting, then each (they are a handful long) by insertion.  From G.he and G.n_vertices.
void graph_rows(HostGraph& G)
{
    const size_t nH = G.he.size(), nV = (size_t)G.n_vertices;
    auto rows = [&](bool out, std::vector<uint32_t>& start, std::vector<int32_t>& nb, std::vector<int32_t>& eid) {
        start.assign(nV + 1, 0);
        for (const HostGraph::HEdge& e : G.he) ++start[(out ? e.v : e.w) + 1];
        for (size_t v = 0; v < nV; ++v) start[v + 1] += start[v];
        nb.resize(nH); eid.resize(nH);
        std::vector<uint32_t> fill(start.begin(), start.end() - 1);
        for (size_t i = 0; i < nH; ++i) {                             // in edge-number order: equal neighbours stay in it
            const HostGraph::HEdge& e = G.he[i];
            const uint32_t row = (uint32_t)(out ? e.v : e.w), lo = start[row];
            const int32_t other = out ? e.w : e.v;
            uint32_t at = fill[row]++;
            while (at > lo && nb[at - 1] > other) { nb[at] = nb[at - 1]; eid[at] = eid[at - 1]; --at; }
            nb[at] = other; eid[at] = (int32_t)i;
        }
    };
    rows(true, G.from_start, G.from_v, G.from_e);
    rows(false, G.to_start, G.to_v, G.to_e);
}

// buildHBVFromEdges (HBVFromEdges.cc:244-296).  The numbering is the reference's queue order, so it is one thread's work; it
// is kept to a few hundred nanoseconds an edge (flat tables, no allocation per edge or vertex) because a real genome has a
// hundred times the edges of the random ones the benchmark builds.
void build_hbv(HostGraph& G)
{
    const uint32_t K = G.K, klo = K - 1;
    const size_t nE = G.ce.size();
    G.fwd.assign(nE, -1); G.rev.assign(nE, -1);
    G.he.clear(); G.n_vertices = 0;
    G.from_start.assign(1, 0); G.to_start.assign(1, 0); G.from_v.clear(); G.from_e.clear(); G.to_v.clear(); G.to_e.clear();
    if (!nE) { G.built = true; return; }
    auto view = [&](size_t c, bool rc) { return SeqView{G.bases.data() + G.ce[c].byte_off, G.ce[c].n + K - 1, rc}; };
    const uint64_t n_bytes = G.bases.size();
    // the four vertex keys of a canonical edge: [0] its first and [1] its last K-1 bases read forwards, [2] [3] the same of its
    // reverse complement (rc of the last, rc of the first)
    std::vector<VKey> ends(4 * nE);
    // a palindromic edge is its own reverse complement: it has one orientation (getCanonicalForm == PALINDROME; an
    // edge of odd length never is)
    std::vector<uint8_t> pal(nE, 0);
    std::vector<uint64_t> head(nE);                                  // the first 32 bases as one big-endian word: decides almost every comparison
    for (size_t c = 0; c < nE; ++c) {
        const uint8_t* p = G.bases.data() + G.ce[c].byte_off;
        const uint64_t off = G.ce[c].byte_off, L = G.ce[c].n + K - 1;
        const u128h first = kmer_at(G.bases.data(), n_bytes, 4 * off, klo), last = kmer_at(G.bases.data(), n_bytes, 4 * off + L - klo, klo);
        ends[4 * c] = vkey_of(first); ends[4 * c + 1] = vkey_of(last);
        ends[4 * c + 2] = vkey_of(kmer_rc_h(last, klo)); ends[4 * c + 3] = vkey_of(kmer_rc_h(first, klo));
        if (!(L & 1) && ends[4 * c] == ends[4 * c + 2]) {               // (a palindrome begins as its reverse complement does)
            const SeqView f = view(c, false), r = view(c, true);
            bool same = true;
            for (uint32_t i = 0; i < f.L && same; ++i) same = f[i] == r[i];
            pal[c] = same;
        }
        uint64_t h = 0;
        { const uint64_t lo = (uint64_t)kmer_at(G.bases.data(), n_bytes, 4 * off, 32); const uint32_t m = (uint32_t)std::min<uint64_t>(32, L);
          for (uint32_t i = 0; i < 32; ++i) h = (h << 2) | (i < m ? (lo >> (2 * i)) & 3u : 0u); }
        head[c] = h; (void)p;
    }
    // canonical edge order: length descending, then lexical (BVComp, :106-111)
    std::vector<uint32_t> order(nE);
    for (size_t i = 0; i < nE; ++i) order[i] = (uint32_t)i;
    std::sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) {
        if (G.ce[x].n != G.ce[y].n) return G.ce[x].n > G.ce[y].n;
        if (head[x] != head[y]) return head[x] < head[y];
        const SeqView a = view(x, false), b = view(y, false);
        for (uint32_t i = 32; i < a.L; ++i) { const uint32_t p = a[i], q = b[i]; if (p != q) return p < q; }
        return false;
    });
    // vertices: the distinct (K-1)-mers at the edge ends, both orientations; each lists its incident
    // (edge, orientation) in canonical edge order, forward before reverse, near end before far end (EEComp, :113-121)
    struct Vtx { int32_t id = -1; uint32_t n = 0; uint32_t inc[8]; };  // inc: canonical edge << 1 | rc  (MAX_EDGES = 8, :79)
    std::vector<Vtx> verts;
    verts.reserve(2 * nE + 16);
    struct Slot { VKey k; uint32_t v; };                               // open addressing, v = index into verts, ~0 = free
    uint64_t tsize = 1024; while (tsize < 8 * (uint64_t)nE) tsize <<= 1;     // <= 4 nE keys: load <= 1/2
    std::vector<Slot> table(tsize, Slot{VKey{0, 0}, 0xFFFFFFFFu});
    auto vertex = [&](const VKey& k, bool insert) -> uint32_t {
        for (uint64_t s = vkey_hash(k) & (tsize - 1);; s = (s + 1) & (tsize - 1)) {
            Slot& t = table[s];
            if (t.v == 0xFFFFFFFFu) { if (!insert) throw std::runtime_error("graph numbering met an unknown vertex"); t.k = k; t.v = (uint32_t)verts.size(); verts.emplace_back(); return t.v; }
            if (t.k == k) return t.v;
        }
    };
    // ends[] index of (canonical edge, orientation, near / far end)
    auto end_key = [&](uint32_t c, int rc, int distal) -> const VKey& { return ends[4 * (size_t)c + 2 * rc + distal]; };
    std::vector<uint32_t> end_vtx(4 * nE, 0xFFFFFFFFu);              // the vertex of each: looked up once
    for (uint32_t c : order)
        for (int rc = 0; rc < (pal[c] ? 1 : 2); ++rc)
            for (int distal = 0; distal < 2; ++distal) {
                const uint32_t vi = vertex(end_key(c, rc, distal), true);
                end_vtx[4 * (size_t)c + 2 * rc + distal] = vi;
                Vtx& v = verts[vi];
                if (v.n >= 8) throw std::runtime_error("a vertex with more than 8 incident edge ends (HBVFromEdges.cc:93 asserts the same)");
                v.inc[v.n++] = (c << 1) | (uint32_t)rc;
            }
    const size_t nV = verts.size();
    G.he.reserve(2 * nE);
    int32_t next_v = 0;
    auto done = [&](uint32_t x) { return ((x & 1) ? G.rev : G.fwd)[x >> 1] != -1; };
    std::vector<uint32_t> q;                                           // the queue: everything pushed stays, `qh` is its head
    q.reserve(4 * nE + 16);
    size_t qh = 0;
    for (int round = 0; round < 2; ++round)
        for (uint32_t c0 : order) {
            const uint32_t first = (c0 << 1) | (uint32_t)round;
            if (done(first)) continue;
            q.push_back(first);
            while (qh < q.size()) {
                const uint32_t x = q[qh++];
                if (done(x)) continue;
                const uint32_t c = x >> 1; const bool rc = x & 1;
                // (a palindrome has its one orientation's ends under rc = 0)
                const int r = rc && !pal[c] ? 1 : 0;
                Vtx& a = verts[end_vtx[4 * (size_t)c + 2 * r]];
                if (a.id < 0) a.id = next_v++;
                Vtx& b = verts[end_vtx[4 * (size_t)c + 2 * r + 1]];
                if (b.id < 0) b.id = next_v++;
                const int32_t id = (int32_t)G.he.size();
                G.he.push_back(HostGraph::HEdge{c, (uint8_t)rc, a.id, b.id});
                if (!rc || pal[c]) G.fwd[c] = id;
                if (rc || pal[c]) G.rev[c] = id;
                for (uint32_t i = 0; i < a.n; ++i) if (!done(a.inc[i])) q.push_back(a.inc[i]);
                for (uint32_t i = 0; i < b.n; ++i) if (!done(b.inc[i])) q.push_back(b.inc[i]);
            }
        }
    if ((size_t)next_v != nV) throw std::runtime_error("graph numbering did not reach every vertex");
    G.n_vertices = nV;
    graph_rows(G);
    G.built = true;
}

// ---- files (all little-endian; "BINWRITE" streams as in feudal/BinaryStream.h:33-46)
struct OutFile {
    FILE* f; std::string path;
    explicit OutFile(const std::string& p) : f(fopen(p.c_str(), "wb")), path(p) { if (!f) throw std::runtime_error("cannot create " + p); }
    ~OutFile() { if (f) fclose(f); }
    void raw(const void* p, size_t n) { if (n && fwrite(p, 1, n, f) != n) throw std::runtime_error("short write " + path); }
    template <class T> void pod(T v) { raw(&v, sizeof v); }
    void vec_i32(const std::vector<int32_t>& v) { pod<uint64_t>(v.size()); raw(v.data(), 4 * v.size()); }
    // rows [start[v], start[v + 1]) of `d` as vec<vec<int>> and as MasterVec<SerfVec<int>>
    void vecvec_i32(const std::vector<uint32_t>& start, const std::vector<int32_t>& d)
    { const size_t n = start.size() - 1; pod<uint64_t>(n); for (size_t v = 0; v < n; ++v) { pod<uint64_t>(start[v + 1] - start[v]); raw(d.data() + start[v], 4 * (size_t)(start[v + 1] - start[v])); } }
    void serf_i32(const std::vector<uint32_t>& start, const std::vector<int32_t>& d)
    { const size_t n = start.size() - 1; pod<uint64_t>(n); for (size_t v = 0; v < n; ++v) { pod<uint32_t>(start[v + 1] - start[v]); raw(d.data() + start[v], 4 * (size_t)(start[v + 1] - start[v])); } }
    void close() { FILE* g = f; f = nullptr; if (fclose(g) != 0) throw std::runtime_error("short write " + path); }
};

// packed bases of one HBV edge (forward: the stored bytes; reverse complement: re-packed)
void packed_edge(const HostGraph& G, const HostGraph::HEdge& e, std::vector<uint8_t>* out)
{
    const uint32_t L = G.ce[e.ce].n + G.K - 1, nb = (L + 3) / 4;
    const uint8_t* p = G.bases.data() + G.ce[e.ce].byte_off;
    out->assign(nb, 0);
    if (!e.rc) { memcpy(out->data(), p, nb); return; }
    // reverse complement a byte (four bases) at a time: the bytes in reverse order through a table give the reverse
    // complement of the PADDED sequence -- the complemented pad bases first -- which is then shifted down by the pad.
    // (Base by base, the three files that carry the edges took 4 s for 1.5x10^9 bases.)
    static const std::array<uint8_t, 256> T = [] {
        std::array<uint8_t, 256> t{};
        for (uint32_t b = 0; b < 256; ++b) {
            uint32_t r = 0;
            for (uint32_t i = 0; i < 4; ++i) r |= (3u - ((b >> (2 * i)) & 3u)) << (2 * (3 - i));
            t[b] = (uint8_t)r;
        }
        return t;
    }();
    const uint32_t s = 2u * (4u * nb - L);                              // bits of pad in front after the reversal (0, 2, 4 or 6)
    uint8_t* o = out->data();
    if (s == 0) { for (uint32_t j = 0; j < nb; ++j) o[j] = T[p[nb - 1 - j]]; }
    else {
        uint32_t cur = T[p[nb - 1]];
        for (uint32_t j = 0; j < nb; ++j) {
            const uint32_t nxt = j + 1 < nb ? T[p[nb - 2 - j]] : 0u;
            o[j] = (uint8_t)((cur >> s) | (nxt << (8 - s)));
            cur = nxt;
        }
    }
}

// (stem: "a." for the graph's files, "a.patch." for the patched graph's, dfk_patch.inc)
void write_graph_files(const HostGraph& G, const std::string& dir, const std::string& stem = "a.")
{
    const uint32_t K = G.K;
    const size_t E = G.he.size();
    std::vector<int32_t> to_left(E), to_right(E), kmers(E), inv(E);
    for (size_t e = 0; e < E; ++e) {
        to_left[e] = G.he[e].v; to_right[e] = G.he[e].w; kmers[e] = (int32_t)G.ce[G.he[e].ce].n;
        // Involution (HyperBasevector.cc:668-680) pairs the i-th smallest edge with the i-th smallest reverse complement;
        // the edge set is closed under reverse complement and free of duplicates, so that is "the edge that is my
        // reverse complement": the same canonical edge in the other orientation
        inv[e] = G.he[e].rc ? G.fwd[G.he[e].ce] : G.rev[G.he[e].ce];
    }
    { OutFile f(dir + "/" + stem + "k"); const std::string s = std::to_string(K) + "\n"; f.raw(s.data(), s.size()); f.close(); }
    std::vector<uint8_t> pk;
    auto edges_vec = [&](OutFile& f) {                                   // vec<basevector>: u64 n, per edge u32 length + packed bases (FieldVec::writeBinary)
        f.pod<uint64_t>(E);
        for (size_t e = 0; e < E; ++e) { packed_edge(G, G.he[e], &pk); f.pod<uint32_t>(G.ce[G.he[e].ce].n + K - 1); f.raw(pk.data(), pk.size()); }
    };
    { OutFile f(dir + "/" + stem + "hbv"); f.raw("BINWRITE", 8); f.pod<int32_t>((int32_t)K);            // K | digraphE: from, from_edge_obj, to_edge_obj, edges
      f.vecvec_i32(G.from_start, G.from_v); f.vecvec_i32(G.from_start, G.from_e); f.vecvec_i32(G.to_start, G.to_e); edges_vec(f); f.close(); }
    { OutFile f(dir + "/" + stem + "to_left"); f.raw("BINWRITE", 8); f.vec_i32(to_left); f.close(); }
    { OutFile f(dir + "/" + stem + "to_right"); f.raw("BINWRITE", 8); f.vec_i32(to_right); f.close(); }
    { OutFile f(dir + "/" + stem + "inv"); f.raw("BINWRITE", 8); f.vec_i32(inv); f.close(); }
    { OutFile f(dir + "/" + stem + "hbx"); f.raw("BINWRITE", 8); f.pod<int32_t>((int32_t)K);            // K | digraphEX (DigraphTemplate.h:2593-2599)
      f.serf_i32(G.from_start, G.from_v); f.serf_i32(G.to_start, G.to_v); f.serf_i32(G.from_start, G.from_e); f.serf_i32(G.to_start, G.to_e); edges_vec(f);
      f.vec_i32(to_left); f.vec_i32(to_right); f.close(); }
    { OutFile f(dir + "/" + stem + "kmers"); f.raw("BINWRITE", 8); f.vec_i32(kmers); f.close(); }
    {   // a.fastb: feudal file, var = packed bases, fixed = u32 lengths (feudal/FeudalFileWriter.cc:26-121)
        uint64_t var = 0;
        std::vector<uint64_t> off(E + 1);
        for (size_t e = 0; e < E; ++e) { off[e] = 24 + var; var += (G.ce[G.he[e].ce].n + K - 1 + 3) / 4; }
        off[E] = 24 + var;
        OutFile f(dir + "/" + stem + "fastb");
        struct { uint32_t n; uint8_t flags, szFixed, szX, szA; uint64_t varTab, fixedOff; } h{(uint32_t)E, 1, 4, 16, 1, 24 + var, 24 + var + 8 * (E + 1)};
        static_assert(sizeof h == 24, "feudal control block");
        f.raw(&h, 24);
        for (size_t e = 0; e < E; ++e) { packed_edge(G, G.he[e], &pk); f.raw(pk.data(), pk.size()); }
        f.raw(off.data(), 8 * (E + 1));
        for (size_t e = 0; e < E; ++e) f.pod<uint32_t>(G.ce[G.he[e].ce].n + K - 1);
        f.close();
    }
}

HostGraph* graph_of(dfk_ctx* c);

// The device half: the canonical edges of the `n` entries a part table names (n > 0), into G->ce and G->bases; the k-mer index, the
// edges' records and their bases stay on the device in G->d_index, G->d_recs and G->d_store, and every entry holds its (edge, offset).
// graph_build_typed runs it over the context's dictionary, dfk_patch.inc over a dictionary and a HostGraph of its own.
template <int K>
int graph_edges_typed(dfk_ctx* c, const PartTable& pt, const uint64_t n, HostGraph* G, float* ms_out)
{
    Timer t(c->stream);
    t.start();
    const uint64_t slots = std::max<uint64_t>(1024, (2 * n + 2 + 1) & ~1ull);          // load 1/2 (even: filled eight bytes at a time)
    const unsigned cus = (unsigned)c->prop.multiProcessorCount;
    DevBuf index, ctr, ends, recs, store, d_bad;
    int rc = c->alloc(index, slots * 4, "k-mer index"); if (rc) return rc;
    rc = c->alloc(ctr, 64, "graph counters"); if (rc) return rc;
    rc = c->alloc(d_bad, 16, "graph check"); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(ctr.p, 0, 64, c->stream));
    HIP_TRY(hipMemsetAsync(d_bad.p, 0, 16, c->stream));
    hipLaunchKernelGGL(k_fill_u64, dim3(4096), dim3(256), 0, c->stream, (uint64_t*)index.p, slots / 2, ~0ull);
    const unsigned grid = (unsigned)std::min<uint64_t>((n + 255) / 256, 32ull * cus);
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_index<K>), dim3(grid), dim3(256), 0, c->stream, pt, n, (uint32_t*)index.p, slots);
    unsigned long long* d_ctr = (unsigned long long*)ctr.p;                    // [0] edges, [1] bytes, [2] ends, [3] list fill, [4] [5] the walks' cursors
    hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_classify<K>), dim3(grid), dim3(256), 0, c->stream, pt, n, (const uint32_t*)index.p, slots, d_ctr + 2);
    HIP_TRY(hipGetLastError());
    uint64_t h[8] = {};
    HIP_TRY(hipMemcpyAsync(h, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t n_ends = h[2];
    TRACE("graph: %llu k-mers, %llu edge ends", (unsigned long long)n, (unsigned long long)n_ends);
    rc = c->alloc(ends, std::max<uint64_t>(1, n_ends) * 4, "edge ends"); if (rc) return rc;
    const unsigned lgrid = (unsigned)std::min<uint64_t>((n + 2047) / 2048, 16ull * cus);
    hipLaunchKernelGGL(k_graph_list, dim3(lgrid), dim3(256), 0, c->stream, pt, n, false, (uint32_t*)ends.p, n_ends, d_ctr + 3);
    // every edge has one or two ends; cycles (pass C) add at most one record per member, reserved separately
    rc = c->alloc(recs, std::max<uint64_t>(1, n_ends) * sizeof(EdgeRec), "edge records"); if (rc) return rc;
    DevBuf info;
    rc = c->alloc(info, std::max<uint64_t>(1, n_ends) * 8, "edge of each end"); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(info.p, 0xFF, std::max<uint64_t>(1, n_ends) * 8, c->stream));
    uint64_t rec_cap = n_ends;
    const uint32_t max_steps = 0x00FFFFFFu;                                   // KDef::MAX_OFFSET: an edge holds fewer than 2^24 k-mers
    if (n_ends) {
        const unsigned wgrid = (unsigned)std::min<uint64_t>((n_ends + 255) / 256, 8ull * cus);   // what is resident; the cursor deals the rest
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_walk_count<K>), dim3(wgrid), dim3(256), 0, c->stream, pt,
                           (const uint32_t*)ends.p, n_ends, (EdgeRec*)recs.p, rec_cap, (uint2*)info.p, d_ctr, max_steps, (unsigned int*)d_bad.p);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, ctr.p, 64, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    TRACE("graph: the ends walked over %llu entries to find %llu edges", (unsigned long long)h[6], (unsigned long long)h[0]);
    if (h[3] != n_ends) return fail(DFK_E_HIP, "graph: %llu edge ends listed, %llu classified", (unsigned long long)h[3], (unsigned long long)n_ends);
    uint64_t n_edges = h[0], n_bytes = h[1];
    c->release(ends);
    const uint64_t store_bytes = (n_bytes + 3) / 4 * 4 + 4;                   // the bases go in by the 32-bit word
    rc = c->alloc(store, store_bytes, "edge bases"); if (rc) return rc;
    HIP_TRY(hipMemsetAsync(store.p, 0, store_bytes, c->stream));
    if (n_edges) {
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_place<K>), dim3(grid), dim3(256), 0, c->stream, pt, n, (const uint2*)info.p, (EdgeRec*)recs.p, (unsigned int*)d_bad.p);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_bases<K>), dim3(grid), dim3(256), 0, c->stream, pt, n, (const EdgeRec*)recs.p, (unsigned int*)store.p);
        HIP_TRY(hipGetLastError());
    }
    // what has no edge yet lies on branch-free cycles
    HIP_TRY(hipMemsetAsync(d_ctr + 3, 0, 8, c->stream));
    hipLaunchKernelGGL(k_graph_list, dim3(lgrid), dim3(256), 0, c->stream, pt, n, true, (uint32_t*)nullptr, (uint64_t)0, d_ctr + 3);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(h, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const uint64_t n_members = h[3];
    c->release(info);
    if (n_members) {
        TRACE("graph: %llu k-mers on branch-free cycles", (unsigned long long)n_members);
        DevBuf members, recs2, store2;
        rc = c->alloc(members, n_members * 4, "cycle members"); if (rc) return rc;
        HIP_TRY(hipMemsetAsync(d_ctr + 3, 0, 8, c->stream));
        hipLaunchKernelGGL(k_graph_list, dim3(lgrid), dim3(256), 0, c->stream, pt, n, true, (uint32_t*)members.p, n_members, d_ctr + 3);
        // the cycles' records and bases go behind the others: grow both buffers
        rc = c->alloc(recs2, (n_edges + n_members) * sizeof(EdgeRec), "edge records (with cycles)"); if (rc) return rc;
        HIP_TRY(hipMemcpyAsync(recs2.p, recs.p, n_edges * sizeof(EdgeRec), hipMemcpyDeviceToDevice, c->stream));
        const unsigned cgrid = (unsigned)std::min<uint64_t>((n_members + 255) / 256, 32ull * cus);
        hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_cycles<K>), dim3(cgrid), dim3(256), 0, c->stream, pt, (const uint32_t*)index.p, slots,
                           (const uint32_t*)members.p, n_members, (EdgeRec*)recs2.p, n_edges + n_members, d_ctr, max_steps, (unsigned int*)d_bad.p);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(h, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        const uint64_t n_edges2 = h[0], n_bytes2 = h[1];
        rc = c->alloc(store2, std::max<uint64_t>(1, n_bytes2), "edge bases (with cycles)"); if (rc) return rc;
        HIP_TRY(hipMemsetAsync(store2.p, 0, std::max<uint64_t>(1, n_bytes2), c->stream));
        HIP_TRY(hipMemcpyAsync(store2.p, store.p, n_bytes, hipMemcpyDeviceToDevice, c->stream));
        if (n_edges2 > n_edges) {
            const unsigned wgrid = (unsigned)std::min<uint64_t>((n_edges2 - n_edges + 255) / 256, 32ull * cus);
            HIP_TRY(hipMemsetAsync(d_ctr + 5, 0, 8, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_graph_walk_write<K>), dim3(wgrid), dim3(256), 0, c->stream, pt,
                               (EdgeRec*)recs2.p, n_edges, n_edges2, (uint8_t*)store2.p, d_ctr + 5, (unsigned int*)d_bad.p);
        }
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->release(members); c->release(recs); c->release(store);
        recs = recs2; store = store2; n_edges = n_edges2; n_bytes = n_bytes2;
        // every k-mer must be on an edge now
        HIP_TRY(hipMemsetAsync(d_ctr + 3, 0, 8, c->stream));
        hipLaunchKernelGGL(k_graph_list, dim3(lgrid), dim3(256), 0, c->stream, pt, n, true, (uint32_t*)nullptr, (uint64_t)0, d_ctr + 3);
        HIP_TRY(hipMemcpyAsync(h, ctr.p, 32, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (h[3]) return fail(DFK_E_HIP, "graph: %llu k-mers were left without an edge", (unsigned long long)h[3]);
    }
    hipLaunchKernelGGL(k_graph_finalize, dim3(grid), dim3(256), 0, c->stream, pt, n);      // the entries' pad words back to 0
    HIP_TRY(hipGetLastError());
    unsigned int bad = 0;
    HIP_TRY(hipMemcpy(&bad, d_bad.p, 4, hipMemcpyDeviceToHost));
    if (bad & 1u) return fail(DFK_E_HIP, "graph: a walk left the dictionary (contexts and k-mers disagree)");
    if (bad & 4u) return fail(DFK_E_HIP, "graph: a k-mer was walked over by an end that found no edge");
    if (bad & 2u) return fail(DFK_E_ARG, "graph: an edge of 2^24 k-mers or more (the reference's KDef::MAX_OFFSET, kmers/ReadPather.h:123, refuses it too)");
    // to the host: records and bases
    std::vector<EdgeRec> hrec(n_edges);
    if (n_edges) HIP_TRY(hipMemcpy(hrec.data(), recs.p, n_edges * sizeof(EdgeRec), hipMemcpyDeviceToHost));
    G->bases.resize(n_bytes);
    if (n_bytes) HIP_TRY(hipMemcpy(G->bases.data(), store.p, n_bytes, hipMemcpyDeviceToHost));
    G->ce.resize(n_edges);
    uint64_t kmers_on_edges = 0;
    uint32_t longest = 0;
    for (uint64_t e = 0; e < n_edges; ++e) { G->ce[e] = GraphEdge{hrec[e].n, hrec[e].byte_off}; kmers_on_edges += hrec[e].n; longest = std::max(longest, hrec[e].n); }
    TRACE("graph: the longest edge has %u k-mers", longest);
    c->release(ctr); c->release(d_bad);
    G->d_index = index; G->index_slots = slots; G->d_recs = recs; G->d_store = store;     // kept: read pathing looks k-mers up and compares bases
    *ms_out = t.stop();
    if (kmers_on_edges != n) return fail(DFK_E_HIP, "graph: the edges hold %llu k-mers, the dictionary %llu", (unsigned long long)kmers_on_edges, (unsigned long long)n);
    return 0;
}

template <int K>
int graph_build_typed(dfk_ctx* c, HostGraph* G)
{
    const uint64_t n = c->n_solid;
    G->K = K; G->ce.clear(); G->bases.clear(); G->built = false;
    if (G->paths) { G->paths_free(G->paths); G->paths = nullptr; }
    c->release(G->d_index); c->release(G->d_recs); c->release(G->d_store); c->release(G->d_filter); G->filter_words = 0;
    if (n >= 0xFFFFFFFFull) return fail(DFK_E_ARG, "the edge builder indexes k-mers with 32 bits: %llu solid k-mers", (unsigned long long)n);
    if (c->parts.size() > (size_t)GRAPH_MAX_PARTS) return fail(DFK_E_ARG, "more than %d dictionary parts", GRAPH_MAX_PARTS);
    if (!n) { build_hbv(*G); return 0; }
    PartTable pt{};
    pt.n_parts = 0;
    uint64_t at = 0;
    for (const dfk_ctx::Part& p : c->parts) { if (!p.n) continue; pt.start[pt.n_parts] = at; pt.ptr[pt.n_parts] = (uint4*)p.buf.p; ++pt.n_parts; at += p.n; }
    pt.start[pt.n_parts] = at;
    float ms_edges = 0;
    if (int rc = graph_edges_typed<K>(c, pt, n, G, &ms_edges)) return rc;
    // The filter the pather puts in front of the index (two bytes a k-mer, 0.1-0.2 s of scattered atomicOr at configs[1]) needs
    // the dictionary's keys and nothing of the graph: it is made NOW, on the device, while the host numbers vertices and edges
    // -- when the reads the count kept say how much room the pathing will want (otherwise dfk_paths_build makes it).
    if (!getenv("DFK_NO_FILTER") && c->kept[0] && c->kept_n_reads) {
        const uint64_t words = std::max<uint64_t>(64, n / 2), free_then = c->largest_allocatable() + c->good_len.bytes;   // (the count's goodLens go when the pathing starts)
        DevBuf f;
        if (free_then > words * 4 + c->kept_n_reads * 18 + (4ull << 30) && c->alloc(f, words * 4, "k-mer filter") == 0) {
            HIP_TRY(hipMemsetAsync(f.p, 0, words * 4, c->stream));
            hipLaunchKernelGGL(HIP_KERNEL_NAME(k_filter_build<K>), dim3((unsigned)std::min<uint64_t>((n + 255) / 256, 32ull * (unsigned)c->prop.multiProcessorCount)), dim3(256), 0, c->stream,
                               pt, n, (uint32_t*)f.p, words);
            HIP_TRY(hipGetLastError());
            G->d_filter = f; G->filter_words = words;
        }
    }
    const auto t0 = std::chrono::steady_clock::now();
    build_hbv(*G);
    const float ms_hbv = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    c->st.reserved[1] = (uint64_t)(ms_edges * 1000.0f);                       // microseconds: edges on the device, numbering on the host
    c->st.reserved[2] = (uint64_t)(ms_hbv * 1000.0f);
    TRACE("graph: %llu canonical edges in %.1f ms, %llu vertices and %zu edges numbered in %.1f ms", (unsigned long long)G->ce.size(), ms_edges,
          (unsigned long long)G->n_vertices, G->he.size(), ms_hbv);
    c->sorted_ok = c->sorted_pre_ok = false;                                   // the entries now carry (edge, offset)
    return 0;
}

} // namespace

struct dfk_graph_holder { HostGraph g; };

namespace {
void graph_delete(void* p) { delete static_cast<dfk_graph_holder*>(p); }
HostGraph* graph_of(dfk_ctx* c)
{
    if (!c->graph_state) { c->graph_state = new dfk_graph_holder; c->graph_state_free = graph_delete; }
    return &static_cast<dfk_graph_holder*>(c->graph_state)->g;
}
}

extern "C" {

int dfk_graph_build(dfk_ctx* c)
{
    return guarded([&]() -> int {
    if (!c || !c->have) return fail(DFK_E_STATE, "no completed count");
    if (c->shard_world > 1 && c->shard_state) return fail(DFK_E_STATE, "the graph is built from a whole dictionary (single-GPU count)");
    HIP_TRY(hipSetDevice(c->device));
    HostGraph* G = graph_of(c);
    const uint64_t mark = c->alloc_seq;
    int rc;
    try {
        switch (c->cfg.K) {
        case 40: rc = graph_build_typed<40>(c, G); break;
        case 48: rc = graph_build_typed<48>(c, G); break;
        default: rc = graph_build_typed<60>(c, G); break;
        }
    } catch (const std::runtime_error& e) { rc = fail(DFK_E_HIP, "%s", e.what()); }
    if (rc) { (void)hipStreamSynchronize(c->stream); c->release_since(mark); G->built = false; G->d_index = G->d_recs = G->d_store = G->d_filter = DevBuf{}; G->filter_words = 0; }
    return rc;
    });
}

int dfk_graph_stats(dfk_ctx* c, uint64_t* n_canonical_edges, uint64_t* n_vertices, uint64_t* n_edges)
{
    if (!c || !c->graph_state || !graph_of(c)->built) return fail(DFK_E_STATE, "no graph: call dfk_graph_build");
    const HostGraph* G = graph_of(c);
    if (n_canonical_edges) *n_canonical_edges = G->ce.size();
    if (n_vertices) *n_vertices = G->n_vertices;
    if (n_edges) *n_edges = G->he.size();
    return 0;
}

int dfk_graph_write(dfk_ctx* c, const char* dir)
{
    return guarded([&]() -> int {
    if (!c || !dir) return fail(DFK_E_ARG, "null argument");
    if (!c->graph_state || !graph_of(c)->built) return fail(DFK_E_STATE, "no graph: call dfk_graph_build");
    try { write_graph_files(*graph_of(c), dir); }
    catch (const std::runtime_error& e) { return fail(DFK_E_ARG, "%s", e.what()); }
    return 0;
    });
}

} // extern "C"
