// dots_coarsen: half-edge-collapse decimation of a triangle mesh on the host (no HIP calls: this translation unit is plain C++17 and
// also compiles with g++ -x c++).  dots_socp_amd/meshes.py: coarsen(backend="python") is the specification and states the rules; the
// arithmetic below is written in the same order of operations, so both return the same arrays.
#include "../../include/dots_socp_hip.h"

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <iterator>
#include <queue>
#include <string>
#include <tuple>
#include <utility>
#include <vector>

namespace dots {
void set_error(const std::string &msg);
}

struct dots_coarse_mesh {
    std::vector<int32_t> kept, tri;
};

namespace {

constexpr double COS_BOUNDARY_TURN = 0.7071067811865476;      // cos(pi / 4)
constexpr double MIN_NORMAL_COSINE = 0.2;

struct Vec3 {
    double x, y, z;
};
inline Vec3 sub(const Vec3 &a, const Vec3 &b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline double dot(const Vec3 &a, const Vec3 &b) { return (a.x * b.x + a.y * b.y) + a.z * b.z; }
inline double norm(const Vec3 &a) { return std::sqrt((a.x * a.x + a.y * a.y) + a.z * a.z); }
inline Vec3 cross(const Vec3 &a, const Vec3 &b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }

using Key = std::tuple<double, int32_t, int32_t>;      // (length, a, b), a < b
using Heap = std::priority_queue<Key, std::vector<Key>, std::greater<Key>>;

struct Coarsener {
    int32_t V, F;
    const Vec3 *P;
    std::vector<int32_t> T;                    // [F][3], rewritten by the collapses
    std::vector<std::vector<int32_t>> inc;     // the live triangles around every vertex
    std::vector<char> alive_v, alive_t;

    bool holds(int32_t f, int32_t w) const { return T[3 * f] == w || T[3 * f + 1] == w || T[3 * f + 2] == w; }
    Vec3 normal(int32_t p0, int32_t p1, int32_t p2) const { return cross(sub(P[p1], P[p0]), sub(P[p2], P[p0])); }
    Key key(int32_t a, int32_t b) const {
        if (b < a) std::swap(a, b);
        return Key(norm(sub(P[a], P[b])), a, b);
    }
    // the neighbours of x, ascending, every one once
    void neighbours(int32_t x, std::vector<int32_t> &out) const {
        out.clear();
        for (int32_t f : inc[x])
            for (int k = 0; k < 3; ++k)
                if (T[3 * f + k] != x) out.push_back(T[3 * f + k]);
        std::sort(out.begin(), out.end());
        out.erase(std::unique(out.begin(), out.end()), out.end());
    }
    bool adjacent(int32_t a, int32_t b) const {
        for (int32_t f : inc[a])
            if (holds(f, b)) return true;
        return false;
    }

    std::vector<int32_t> nu, nv, common, opposite, all, edge_t, around;

    bool allowed(int32_t u, int32_t v) {
        edge_t.clear();
        for (int32_t f : inc[v])
            if (holds(f, u)) edge_t.push_back(f);
        if (edge_t.size() < 1 || edge_t.size() > 2) return false;
        neighbours(u, nu);
        neighbours(v, nv);
        common.clear();
        std::set_intersection(nu.begin(), nu.end(), nv.begin(), nv.end(), std::back_inserter(common));
        opposite.clear();
        for (int32_t f : edge_t)
            for (int k = 0; k < 3; ++k)
                if (T[3 * f + k] != u && T[3 * f + k] != v) opposite.push_back(T[3 * f + k]);
        std::sort(opposite.begin(), opposite.end());
        opposite.erase(std::unique(opposite.begin(), opposite.end()), opposite.end());
        if (common != opposite) return false;
        // the neighbours of v that share one triangle with it only: its boundary neighbours
        around.clear();
        for (int32_t f : inc[v])
            for (int k = 0; k < 3; ++k)
                if (T[3 * f + k] != v) around.push_back(T[3 * f + k]);
        std::sort(around.begin(), around.end());
        int32_t boundary[2] = {-1, -1};
        size_t n_boundary = 0;
        for (size_t i = 0; i < around.size();) {
            size_t j = i;
            while (j < around.size() && around[j] == around[i]) ++j;
            if (j - i == 1) {
                if (n_boundary < 2) boundary[n_boundary] = around[i];
                ++n_boundary;
            }
            i = j;
        }
        if (n_boundary > 0) {
            if (edge_t.size() != 1 || n_boundary != 2) return false;
            const Vec3 a = sub(P[v], P[boundary[0]]), b = sub(P[boundary[1]], P[v]);
            if (!(dot(a, b) >= (COS_BOUNDARY_TURN * norm(a)) * norm(b))) return false;
        } else {
            all.clear();
            std::set_union(nu.begin(), nu.end(), nv.begin(), nv.end(), std::back_inserter(all));
            size_t n = 0;
            for (int32_t w : all)
                if (w != u && w != v) ++n;
            if (n < 3) return false;
        }
        for (int32_t f : inc[v]) {
            if (std::find(edge_t.begin(), edge_t.end(), f) != edge_t.end()) continue;
            int32_t p[3], q[3];
            for (int k = 0; k < 3; ++k) {
                p[k] = T[3 * f + k];
                q[k] = p[k] == v ? u : p[k];
            }
            const Vec3 n_old = normal(p[0], p[1], p[2]), n_new = normal(q[0], q[1], q[2]);
            const double length = norm(n_new);
            if (!(length > 0.0) || !(dot(n_old, n_new) >= (MIN_NORMAL_COSINE * norm(n_old)) * length)) return false;
        }
        return true;
    }

    void collapse(int32_t u, int32_t v) {
        const std::vector<int32_t> of_v = inc[v];
        for (int32_t f : of_v) {
            if (!holds(f, u)) continue;
            alive_t[f] = 0;
            for (int k = 0; k < 3; ++k) {
                std::vector<int32_t> &l = inc[T[3 * f + k]];
                l.erase(std::find(l.begin(), l.end(), f));
            }
        }
        for (int32_t f : inc[v]) {
            for (int k = 0; k < 3; ++k)
                if (T[3 * f + k] == v) T[3 * f + k] = u;
            inc[u].push_back(f);
        }
        inc[v].clear();
        alive_v[v] = 0;
    }

    void all_edges(Heap &heap) {
        std::vector<int32_t> nb;
        for (int32_t a = 0; a < V; ++a) {
            if (!alive_v[a]) continue;
            neighbours(a, nb);
            for (int32_t b : nb)
                if (a < b) heap.push(key(a, b));
        }
    }

    void run(int32_t target) {
        Heap heap;
        all_edges(heap);
        int32_t live = V;
        bool collapsed = false;
        std::vector<int32_t> nb;
        while (live > target) {
            if (heap.empty()) {
                if (!collapsed) break;      // a whole refill without a collapse: what was reached is the result
                all_edges(heap);
                collapsed = false;
                continue;
            }
            const Key top = heap.top();
            heap.pop();
            const int32_t a = std::get<1>(top), b = std::get<2>(top);
            if (!alive_v[a] || !alive_v[b] || !adjacent(a, b)) continue;
            for (int dir = 0; dir < 2; ++dir) {
                const int32_t u = dir ? b : a, v = dir ? a : b;
                if (!allowed(u, v)) continue;
                collapse(u, v);
                --live;
                collapsed = true;
                neighbours(u, nb);
                for (int32_t w : nb) heap.push(key(u, w));
                break;
            }
        }
    }
};

int refuse(const char *what) {
    dots::set_error(std::string("coarsen: ") + what);
    return DOTS_ERR_ARGUMENT;
}

}  // namespace

extern "C" {

int dots_coarsen(int32_t V, int32_t F, const double *xyz, const int32_t *tri, int32_t n_target, dots_coarse_mesh **out) {
    if (V < 1 || F < 1 || !xyz || !tri || !out || n_target < 1) return refuse("bad argument");
    for (int64_t i = 0; i < (int64_t)F * 3; ++i)
        if (tri[i] < 0 || tri[i] >= V) return refuse("triangle index out of range");
    for (int64_t i = 0; i < (int64_t)V * 3; ++i)
        if (!std::isfinite(xyz[i])) return refuse("non-finite coordinates");
    const Vec3 *P = reinterpret_cast<const Vec3 *>(xyz);
    for (int32_t f = 0; f < F; ++f)
        if (!(norm(cross(sub(P[tri[3 * f + 1]], P[tri[3 * f]]), sub(P[tri[3 * f + 2]], P[tri[3 * f]]))) > 0.0)) return refuse("a triangle of zero area");
    {
        std::vector<std::pair<int32_t, int32_t>> directed((size_t)F * 3), undirected((size_t)F * 3);
        for (int32_t f = 0; f < F; ++f)
            for (int k = 0; k < 3; ++k) {
                const int32_t a = tri[3 * f + k], b = tri[3 * f + (k + 1) % 3];
                directed[(size_t)3 * f + k] = {a, b};
                undirected[(size_t)3 * f + k] = {std::min(a, b), std::max(a, b)};
            }
        std::sort(undirected.begin(), undirected.end());
        for (size_t i = 2; i < undirected.size(); ++i)
            if (undirected[i] == undirected[i - 2]) return refuse("an edge with more than two triangles");
        std::sort(directed.begin(), directed.end());
        for (size_t i = 1; i < directed.size(); ++i)
            if (directed[i] == directed[i - 1]) return refuse("two triangles cross an edge in the same direction");
    }
    Coarsener c;
    c.V = V;
    c.F = F;
    c.P = P;
    c.T.assign(tri, tri + (size_t)F * 3);
    c.inc.resize((size_t)V);
    for (int32_t f = 0; f < F; ++f)
        for (int k = 0; k < 3; ++k) c.inc[(size_t)tri[3 * f + k]].push_back(f);
    c.alive_v.assign((size_t)V, 1);
    c.alive_t.assign((size_t)F, 1);
    c.run(n_target);
    dots_coarse_mesh *m = new dots_coarse_mesh;
    for (int32_t v = 0; v < V; ++v)
        if (c.alive_v[v]) m->kept.push_back(v);
    for (int32_t f = 0; f < F; ++f)
        if (c.alive_t[f]) m->tri.insert(m->tri.end(), c.T.begin() + (size_t)3 * f, c.T.begin() + (size_t)3 * f + 3);
    *out = m;
    return DOTS_OK;
}

int64_t dots_coarsen_vertices(const dots_coarse_mesh *m) { return m ? (int64_t)m->kept.size() : -1; }
int64_t dots_coarsen_triangles(const dots_coarse_mesh *m) { return m ? (int64_t)(m->tri.size() / 3) : -1; }
int dots_coarsen_copy(const dots_coarse_mesh *m, int32_t *kept, int32_t *tri) {
    if (!m || !kept || !tri) {
        dots::set_error("coarsen_copy: null argument");
        return DOTS_ERR_ARGUMENT;
    }
    std::copy(m->kept.begin(), m->kept.end(), kept);
    std::copy(m->tri.begin(), m->tri.end(), tri);
    return DOTS_OK;
}
void dots_coarsen_free(dots_coarse_mesh *m) { delete m; }

}  // extern "C"
