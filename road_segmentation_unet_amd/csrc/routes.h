// Launch prototypes of the network distances and the path-length score (routes.hip; include/rsu_routes.h).
#pragma once
#include "rsu_common.h"

constexpr int RT_MAX_SIDE = 1024;     // largest H and W
constexpr int RT_MAX_NODES = 1024;    // largest max_nodes
constexpr int RT_MAX_EDGES = 65536;   // largest max_edges
constexpr int RT_INF = 0x3fffffff;    // no path
constexpr int RT_Q = 65536;           // the unit of a pair's contribution
// the rounds of the blocked Floyd-Warshall: ceil(max_nodes / 64)
int rt_rounds(int max_nodes);
// ws: the root counts int32 [N][ceil(H W / 256)], then the zone sums int32 [N][max_nodes][3]
size_t rt_ws_bytes(int N, int H, int W, int max_nodes);
// the launches of one rt_graph_routes call: count, scan, place, fill, sums, close, edges, the first diagonal tile, then two per round
int rt_launches(int max_nodes);
hipError_t rt_graph_routes(const int32_t* node_map, const int32_t* edges, const int32_t* counts, int side, int max_edges, int max_nodes,
                           int32_t* nodes, int32_t* dist, int32_t* info, void* ws, int N, int H, int W, hipStream_t st);
hipError_t rt_route_score(const int32_t* nodes_a, const int32_t* dist_a, const int32_t* info_a, const int32_t* nodes_b, const int32_t* dist_b,
                          const int32_t* info_b, int max_nodes, int slack, int32_t* match, unsigned long long* acc, int N, hipStream_t st);
