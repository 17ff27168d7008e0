// cluster_tree.h -- the host half of HDBSCAN* (DESIGN.md section 19): from the n - 1 edges of a minimum spanning tree of the
// mutual-reachability graph to flat labels.  Plain C++17, no HIP: single-linkage hierarchy by union-find (one node per weight level), condensed tree, stabilities,
// excess-of-mass selection, cluster_selection_epsilon, allow_single_cluster, labels numbered by smallest member.
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <limits>
#include <numeric>
#include <vector>

namespace mirast {

enum ClTreeStatus { CL_TREE_OK = 0, CL_TREE_BAD_COUNT, CL_TREE_BAD_INDEX, CL_TREE_BAD_WEIGHT, CL_TREE_CYCLE };

namespace cltree {

struct Cluster {
    int parent;         // -1 for the root cluster
    double birth;       // lambda = 1 / distance at which it split off its parent (0 for the root)
    double stability;
    int size;
    int first_child, n_children;   // the clusters it splits into are created together, one after the other
};

inline int find(std::vector<int>& up, int x)
{
    int r = x;
    while (up[r] != r) r = up[r];
    while (up[x] != r) {
        const int nx = up[x];
        up[x] = r;
        x = nx;
    }
    return r;
}

}  // namespace cltree

// labels[n]: -1 for noise, else 0 .. K-1 in ascending order of each cluster's smallest member.  Returns a ClTreeStatus; labels and
// n_clusters are written only with CL_TREE_OK.  n >= 1, min_cluster_size >= 2, epsilon >= 0 are the caller's to check.
inline int cluster_labels_from_mst(int n, int n_edges, const int* edge_a, const int* edge_b, const float* edge_w, int min_cluster_size,
                                   double epsilon, bool allow_single_cluster, int* labels, int* n_clusters)
{
    using cltree::Cluster;
    if (n_edges != n - 1) return CL_TREE_BAD_COUNT;
    for (int e = 0; e < n_edges; e++) {
        if (edge_a[e] < 0 || edge_a[e] >= n || edge_b[e] < 0 || edge_b[e] >= n) return CL_TREE_BAD_INDEX;
        if (!(edge_w[e] >= 0.f) || std::isinf(edge_w[e])) return CL_TREE_BAD_WEIGHT;
    }
    // 1. edges by (weight, lower end, higher end): the result does not depend on the order they arrive in
    std::vector<int> order(n_edges);
    std::iota(order.begin(), order.end(), 0);
    auto lo = [&](int e) { return std::min(edge_a[e], edge_b[e]); };
    auto hi = [&](int e) { return std::max(edge_a[e], edge_b[e]); };
    std::sort(order.begin(), order.end(), [&](int p, int q) {
        if (edge_w[p] != edge_w[q]) return edge_w[p] < edge_w[q];
        if (lo(p) != lo(q)) return lo(p) < lo(q);
        if (hi(p) != hi(q)) return hi(p) < hi(q);
        return p < q;
    });
    // single-linkage hierarchy BY LEVELS: nodes 0 .. n-1 are the points; every further node is one component at one distinct weight,
    // with all the components that weight joins as its children.  Edges of equal weight are one level, so neither their order nor
    // which of several minimum spanning trees arrived changes the hierarchy (the components below every weight are the same).
    const int n_nodes = 2 * n - 1;
    std::vector<int> size(n_nodes, 1), first(n_nodes, -1), last(n_nodes, -1), next(n_nodes, -1), level(n_nodes, -1), up(n), node_of(n);
    std::vector<double> dist(n_nodes, 0.0);
    std::iota(up.begin(), up.end(), 0);
    std::iota(node_of.begin(), node_of.end(), 0);
    int used = n, group = 0;
    for (int k = 0; k < n_edges; k++) {
        const int e = order[k];
        if (k > 0 && edge_w[e] != edge_w[order[k - 1]]) group++;
        const int ra = cltree::find(up, edge_a[e]), rb = cltree::find(up, edge_b[e]);
        if (ra == rb) return CL_TREE_CYCLE;
        int na = node_of[ra], nb = node_of[rb];
        if (level[nb] == group && level[na] != group) std::swap(na, nb);
        int target = na;
        if (level[na] != group) {            // neither is of this level: a new node over both
            target = used++;
            dist[target] = (double)edge_w[e];
            level[target] = group;
            size[target] = size[na] + size[nb];
            first[target] = na;
            next[na] = nb;
            last[target] = nb;
        } else if (level[nb] == group) {     // both of this level: one node, the children of both
            next[last[na]] = first[nb];
            last[na] = last[nb];
            size[na] += size[nb];
        } else {                             // nb joins the node of this level
            next[last[na]] = nb;
            last[na] = nb;
            size[na] += size[nb];
        }
        up[ra] = rb;
        node_of[rb] = target;
    }
    const int root = node_of[cltree::find(up, 0)];
    std::fill(labels, labels + n, -1);
    *n_clusters = 0;
    if (n < min_cluster_size || n < 2) return CL_TREE_OK;

    // 2. condensed tree, top down: every node belongs to a cluster; a child smaller than min_cluster_size falls out of it, two or more
    // children of at least that size are new clusters, a single one carries the cluster on
    const double INF = std::numeric_limits<double>::infinity();
    std::vector<Cluster> cl;
    cl.push_back({-1, 0.0, 0.0, n, -1, 0});
    std::vector<int> point_cluster(n, 0);
    std::vector<double> point_lambda(n, 0.0);
    std::vector<std::pair<int, int>> stack;   // (node, cluster)
    std::vector<int> walk;
    stack.push_back({root, 0});
    auto drop = [&](int top, int c, double lambda) {   // every point below `top` leaves cluster c at lambda
        walk.assign(1, top);
        while (!walk.empty()) {
            const int v = walk.back();
            walk.pop_back();
            if (v < n) {
                point_cluster[v] = c;
                point_lambda[v] = lambda;
            } else {
                for (int ch = first[v]; ch >= 0; ch = next[ch]) walk.push_back(ch);
            }
        }
    };
    while (!stack.empty()) {
        const auto [node, c] = stack.back();
        stack.pop_back();
        const double lambda = dist[node] > 0.0 ? 1.0 / dist[node] : INF;
        int big = 0, leaving = size[node];
        for (int ch = first[node]; ch >= 0; ch = next[ch]) big += size[ch] >= min_cluster_size;
        if (big == 1)
            for (int ch = first[node]; ch >= 0; ch = next[ch])
                if (size[ch] >= min_cluster_size) leaving -= size[ch];   // it carries the cluster on
        cl[c].stability += (lambda - cl[c].birth) * leaving;
        if (big >= 2) {
            cl[c].first_child = (int)cl.size();
            cl[c].n_children = big;
        }
        for (int ch = first[node]; ch >= 0; ch = next[ch]) {
            if (size[ch] < min_cluster_size) drop(ch, c, lambda);
            else if (big == 1) stack.push_back({ch, c});
            else {
                stack.push_back({ch, (int)cl.size()});
                cl.push_back({c, lambda, 0.0, size[ch], -1, 0});
            }
        }
    }
    // 3. excess of mass, children before parents (a child has a higher index than its parent)
    const int nc = (int)cl.size();
    std::vector<char> chosen(nc, 0);
    for (int c = nc - 1; c >= 0; c--) {
        if (c == 0 && !allow_single_cluster) break;
        double below = 0.0;
        for (int k = 0; k < cl[c].n_children; k++) below += cl[cl[c].first_child + k].stability;
        if (below > cl[c].stability) cl[c].stability = below;
        else chosen[c] = 1;
    }
    // a chosen cluster wins over every chosen cluster below it
    auto keep_topmost = [&]() {
        std::vector<char> covered(nc, 0);
        for (int c = 1; c < nc; c++) {
            covered[c] = covered[cl[c].parent] || chosen[cl[c].parent];
            if (covered[c]) chosen[c] = 0;
        }
    };
    keep_topmost();
    // 4. cluster_selection_epsilon: a chosen cluster born below epsilon is replaced by its lowest ancestor born above it
    const bool root_alone = chosen[0] != 0;
    if (epsilon != 0.0 && nc > 1 && !root_alone) {
        auto birth_eps = [&](int c) { return 1.0 / cl[c].birth; };
        std::vector<char> next(nc, 0);
        for (int c = 1; c < nc; c++) {
            if (!chosen[c]) continue;
            int cur = c;
            if (birth_eps(c) < epsilon) {
                for (;;) {
                    const int p = cl[cur].parent;
                    if (p == 0) {
                        if (allow_single_cluster) cur = 0;
                        break;
                    }
                    cur = p;
                    if (birth_eps(p) > epsilon) break;
                }
            }
            next[cur] = 1;
        }
        chosen = next;
        keep_topmost();
    }
    // 5. labels: a point belongs to the nearest chosen cluster at or above the one it fell out of
    std::vector<int> number(nc, -1);
    int count = 0;
    if (chosen[0]) {
        // the root as the only cluster: a point stays in it while its own lambda reaches the threshold
        double thr = 0.0;
        if (epsilon != 0.0) thr = 1.0 / epsilon;
        else {
            for (int i = 0; i < n; i++)
                if (point_cluster[i] == 0) thr = std::max(thr, point_lambda[i]);
            for (int k = 0; k < cl[0].n_children; k++) thr = std::max(thr, cl[cl[0].first_child + k].birth);
        }
        for (int i = 0; i < n; i++)
            if (point_lambda[i] >= thr) {
                labels[i] = 0;
                count = 1;
            }
    } else {
        for (int i = 0; i < n; i++) {
            int c = point_cluster[i];
            while (c >= 0 && !chosen[c]) c = cl[c].parent;
            if (c < 0) continue;
            if (number[c] < 0) number[c] = count++;   // points in ascending order: numbered by smallest member
            labels[i] = number[c];
        }
    }
    *n_clusters = count;
    return CL_TREE_OK;
}

}  // namespace mirast
