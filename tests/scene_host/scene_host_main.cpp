// Driver of tests/test_scene_host.py: rts_amd/csrc/rts_scene_host.h alone, no HIP.
// One case per input line, tokens separated by blanks:
//   flatten S N M  mesh*M     rts_scene_flatten(meshes, N, S) -- M meshes are handed over (M = -1: a null `meshes`)
//   bounds  S N M  mesh*M     ... and rts_mesh_bounds of every mesh of the flattened scene
//   concat  K                 the first K of the three trees written out below through rts_scene_append_tree (K = 2: the first and the last)
// mesh: n_triangles n_vertices n_normals refl_coeff refr_index  kt t*kt  kv v*kv  kn n*kn -- the three arrays as heap blocks of
// EXACTLY kt / kv / kn elements (-1: a null pointer), whatever the counts say: a read one element outside is a sanitizer report.
// The answer: "key value ..." lines, closed by a line "end".
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <iostream>
#include <memory>
#include <sstream>
#include <string>
#include "rts_scene_host.h"

static char g_err[1024] = "";
void rts_set_error(const char* fmt, ...) { va_list ap; va_start(ap, fmt); vsnprintf(g_err, sizeof(g_err), fmt, ap); va_end(ap); }

template <class T> static void print_u(const char* key, const std::vector<T>& v) { printf("%s", key); for (T x : v) printf(" %llu", (unsigned long long)x); printf("\n"); }
static void print_d(const char* key, const double* v, size_t n) { printf("%s", key); for (size_t i = 0; i < n; i++) printf(" %a", v[i]); printf("\n"); }

struct MeshBlocks { std::unique_ptr<uint32_t[]> t; std::unique_ptr<double[]> v, n; };
template <class T> static std::unique_ptr<T[]> read_block(std::istringstream& in)
{
    long k = 0; in >> k;
    if (k < 0) return nullptr;
    std::unique_ptr<T[]> p(new T[(size_t)k]);
    for (long i = 0; i < k; i++) { std::string tok; in >> tok; p[(size_t)i] = (T)strtod(tok.c_str(), nullptr); }
    return p;
}

static void run_flatten(std::istringstream& in, bool bounds)
{
    int smooth = 0; uint32_t n_targets = 0; long m_given = 0;
    in >> smooth >> n_targets >> m_given;
    std::vector<RtsMesh> meshes; std::vector<MeshBlocks> blocks;
    for (long i = 0; i < m_given; i++) {
        RtsMesh m; memset(&m, 0, sizeof(m));
        in >> m.n_triangles >> m.n_vertices >> m.n_normals >> m.refl_coeff >> m.refr_index;
        MeshBlocks b; b.t = read_block<uint32_t>(in); b.v = read_block<double>(in); b.n = read_block<double>(in);
        m.triangles = b.t.get(); m.vertices = b.v.get(); m.normals = b.n.get();
        meshes.push_back(m); blocks.push_back(std::move(b));
    }
    RtsSceneFlat f; g_err[0] = 0;
    const int rc = rts_scene_flatten(m_given < 0 ? nullptr : meshes.data(), n_targets, smooth != 0, &f);
    printf("rc %d\nerr %s\n", rc, g_err);
    if (rc == RTS_OK) {
        for (const RtsMeshHost& h : f.meshes)
            printf("mesh %u %u %u %u %u %u %a %a %d\n", h.n_tris, h.n_verts, h.n_normals, h.tri_base, h.vert_base, h.normal_base, h.refl_coeff, h.refr_index, h.perface ? 1 : 0);
        print_u("vidx", f.vidx); print_u("nidx", f.nidx); print_u("ptarg", f.ptarg); print_u("vtarg", f.vtarg); print_u("ntarg", f.ntarg);
        print_d("verts", f.verts.data(), f.verts.size()); print_d("normals", f.normals.data(), f.normals.size());
        printf("totals %llu %llu %llu\n", (unsigned long long)f.n_tris, (unsigned long long)f.n_verts, (unsigned long long)f.n_normals);
        if (bounds) for (uint32_t t = 0; t < n_targets; t++) {
            RtsBlasInfo b; memset(&b, 0xff, sizeof(b));               // (whatever was there before is overwritten)
            rts_mesh_bounds(f, t, &b);
            const double v[7] = {b.lo[0], b.lo[1], b.lo[2], b.hi[0], b.hi[1], b.hi[2], b.max_abs};
            print_d("bounds", v, 7);
        }
    }
    printf("end\n");
}

// ---- three per-mesh trees as the host builder leaves them: children (>= 0 node, ~slot, 0x7fffffff unused), leaf slots -> primitives of the mesh
static const int32_t U = 0x7fffffff;
struct Tree { std::vector<RtsNode4> nodes; std::vector<uint32_t> leaf_prim; int32_t root; uint32_t n_prims; };
static RtsNode4 node(int id, int32_t c0, int32_t c1, int32_t c2, int32_t c3)
{
    RtsNode4 n; memset(&n, 0, sizeof(n));
    for (int k = 0; k < 4; k++) { n.lox[k] = (float)(100 * id + k); n.loy[k] = n.lox[k] + 0.25f; n.loz[k] = n.lox[k] + 0.5f; n.hix[k] = n.lox[k] + 10; n.hiy[k] = n.lox[k] + 20; n.hiz[k] = n.lox[k] + 30; }
    n.child[0] = c0; n.child[1] = c1; n.child[2] = c2; n.child[3] = c3;
    return n;
}
static std::vector<Tree> trees()
{
    Tree a; a.nodes = { node(1, 1, ~0, 2, U), node(2, ~1, ~2, U, U), node(3, ~3, ~4, ~5, ~6) }; a.leaf_prim = {0, 1, 2, 1, 3, 4, 0}; a.root = 0; a.n_prims = 5;      // (primitives 0 and 1: two references each)
    Tree b; b.root = -1; b.n_prims = 0;                                       // a mesh without (finite) triangles: no nodes, no root
    Tree c; c.nodes = { node(4, ~0, U, U, U) }; c.leaf_prim = {0}; c.root = 0; c.n_prims = 1;      // a single triangle
    return {a, b, c};
}
static void print_tree(const char* key, const std::vector<RtsNode4>& nodes)
{
    for (const RtsNode4& n : nodes) { uint32_t w[32]; memcpy(w, &n, sizeof(w)); printf("%s", key); for (int i = 0; i < 32; i++) printf(" %u", w[i]); printf("\n"); }
}
static void run_concat(std::istringstream& in)
{
    int k = 0; in >> k;
    std::vector<Tree> all = trees(); std::vector<Tree> use;
    if (k == 2) use = {all[0], all[2]}; else use = all;
    std::vector<RtsNode4> nodes4; std::vector<uint32_t> leaf_prim; uint32_t tri_base = 0;
    for (const Tree& t : use) {
        RtsBlasInfo b; memset(&b, 0, sizeof(b)); b.root = t.root; b.n_nodes = (uint32_t)t.nodes.size(); b.n_leaves = (uint32_t)t.leaf_prim.size();
        printf("in_tree %d %u\n", t.root, tri_base); print_tree("in_node", t.nodes); print_u("in_leaf", t.leaf_prim);
        rts_scene_append_tree(t.nodes, t.leaf_prim, tri_base, &nodes4, &leaf_prim, &b);
        printf("root %d %u %u\n", b.root, b.n_nodes, b.n_leaves);
        tri_base += t.n_prims;
    }
    print_tree("node", nodes4); print_u("leaf", leaf_prim);
    printf("end\n");
}

int main()
{
    std::string line;
    while (std::getline(std::cin, line)) {
        std::istringstream in(line);
        std::string cmd; in >> cmd;
        if (cmd == "flatten") run_flatten(in, false);
        else if (cmd == "bounds") run_flatten(in, true);
        else if (cmd == "concat") run_concat(in);
        else { fprintf(stderr, "unknown case: %s\n", cmd.c_str()); return 2; }
    }
    return 0;
}
