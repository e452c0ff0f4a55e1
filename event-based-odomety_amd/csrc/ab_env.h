// ab_env.h — A/B switches and test hooks of the host side.
//
// The shipped library (libebo_hip.so) reads four documented environment variables and nothing else:
//   EBO_HOST_THREADS, EBO_HOST_SPIN_US   the host LM's worker threads and their spin time (host_pool.h)
//   EBO_EDGE_CS_MB                       cap of the edge loss's direction table (ebo_api.cpp)
//   EBO_LM_NO_AVX2                       scalar band Cholesky in the host LM (host_lm.cpp)
//   EBO_SOLVE_TRACE, EBO_INGEST_TRACE    diagnostics on stderr
// Everything else -- forcing an implementation a launch would not pick at this size, block shapes, ablations,
// the switches the equivalence tests flip -- goes through ab_env() / ab_size(), which look at the environment only
// in the -DEBO_AB build (`make ab` -> libebo_hip_ab.so: what tools/ab/*, the tools' A/B scripts and the tests' `ebo_ab`
// fixture load).  In the shipped build they are constant: one path per call, no knob string in the binary.
// Among them, the space-sweep vote's (ebo_depth.cpp):
//   EBO_DSI_TILE = 0     every tap of k_dsi_vote a global atomic instead of the LDS tile per (patch, plane); read by
//                        ebo_dsi_begin
//   EBO_DSI_PLANES = n   planes per workgroup of k_dsi_vote instead of the count the launch size gives
#pragma once

#include <cstdlib>
#include <cstring>

namespace ebo_ab
{
#ifdef EBO_AB
inline const char* ab_env(const char* name) { return std::getenv(name); }
#else
inline const char* ab_env(const char*) { return nullptr; }
#endif
inline size_t ab_size(const char* name, size_t dflt)
{
	const char* v = ab_env(name);
	if (!v || !*v)
	{
		return dflt;
	}
	return static_cast<size_t>(std::strtoull(v, nullptr, 10));
}
// EBO_EVAL_ORDER = index | light: the launch-order table a load builds (launch_order.h: 1 the identity, 2 lightest
// first; anything else, and always in the shipped build, 0 = heaviest first).  Read when windows or patches are loaded.
inline int ab_launch_order()
{
	const char* v = ab_env("EBO_EVAL_ORDER");
	if (!v)
	{
		return 0;
	}
	return std::strcmp(v, "index") == 0 ? 1 : std::strcmp(v, "light") == 0 ? 2 : 0;
}
// EBO_EVAL_BOX = events | extents: where k_eval3 and k_solve_independent take a unit's bounding box from -- a pass over
// its events, or the load's time-extent table where that gives the box exactly (box_extents.h; the default, and always
// in the shipped build).  Read at every launch.
inline bool ab_box_from_extents()
{
	const char* v = ab_env("EBO_EVAL_BOX");
	return !(v && std::strcmp(v, "events") == 0);
}
}  // namespace ebo_ab
using ebo_ab::ab_box_from_extents;
using ebo_ab::ab_env;
using ebo_ab::ab_launch_order;
using ebo_ab::ab_size;
