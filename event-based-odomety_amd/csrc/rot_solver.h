// rot_solver.h — the three-variable solver of the rotational contrast maximisation (include/ebo.h, rules N1-N5): a
// backtracking gradient descent with Barzilai-Borwein steps, as a reverse-communication state machine over n windows at
// once.  Plain host C++, no HIP (as lockstep.h): what it returns is a function of the numbers it is fed and of nothing
// else.  Compiled without contraction (-ffp-contract=off): every operation below rounds once, in the association written,
// which is what tests/rotation_ref.py restates.
#pragma once

#include <cmath>
#include <cstdint>
#include <vector>

#include "../../include/ebo.h"

namespace ebo
{
class RotSolver
{
public:
	RotSolver(int n, const ebo_rot_solver_opts& o, const double* omega0) : o_(o), w_(static_cast<size_t>(n))
	{
		for (size_t i = 0; i < w_.size(); ++i)
		{
			for (int k = 0; k < 3; ++k)
			{
				w_[i].om[k] = omega0 ? omega0[3 * i + k] : 0.0;
				w_[i].trial[k] = w_[i].om[k];
			}
		}
	}

	static bool optsOk(const ebo_rot_solver_opts& o)
	{
		return std::isfinite(o.first_rate) && o.first_rate > 0.0 && o.c1 > 0.0 && o.c1 < 1.0 && o.max_backtracks >= 1 &&
			   o.step_tol >= 0.0 && o.max_iterations >= 1;
	}

	int size() const { return static_cast<int>(w_.size()); }

	// the points the evaluation is wanted at: omegas [n][3] (a finished window's entry is its result), live [n] = 1 where
	// the window still waits for an evaluation; returns the number of live windows
	int request(double* omegas, uint8_t* live) const
	{
		int n = 0;
		for (size_t i = 0; i < w_.size(); ++i)
		{
			const Win& s = w_[i];
			const bool on = s.phase != kDone;
			for (int k = 0; k < 3; ++k)
			{
				omegas[3 * i + k] = on ? s.trial[k] : s.om[k];
			}
			if (live)
			{
				live[i] = on ? 1 : 0;
			}
			n += on ? 1 : 0;
		}
		return n;
	}

	// r [n], g [n][3]: the objective (V6) and its gradient (V8) at the requested points; entries of finished windows are ignored
	void supply(const double* r, const double* g)
	{
		for (size_t i = 0; i < w_.size(); ++i)
		{
			if (w_[i].phase != kDone)
			{
				step(w_[i], r[i], g + 3 * i);
			}
		}
	}

	void result(double* omegas, ebo_rot_summary* summary) const
	{
		for (size_t i = 0; i < w_.size(); ++i)
		{
			const Win& s = w_[i];
			if (omegas)
			{
				for (int k = 0; k < 3; ++k)
				{
					omegas[3 * i + k] = s.om[k];
				}
			}
			if (summary)
			{
				summary[i].status = s.phase == kDone ? s.status : EBO_ROT_RUNNING;
				summary[i].iterations = s.iterations;
				summary[i].evaluations = s.evaluations;
				summary[i].reserved = 0;
				summary[i].r_initial = s.rInitial;
				summary[i].r_final = s.phase == kFirst ? 0.0 : -s.f;
			}
		}
	}

private:
	enum Phase
	{
		kFirst,
		kTrial,
		kDone
	};
	struct Win
	{
		Phase phase = kFirst;
		int status = EBO_ROT_RUNNING, iterations = 0, evaluations = 0, backtracks = 0;
		double om[3] = {}, trial[3] = {}, gf[3] = {};
		double f = 0.0, alpha = 0.0, slope = 0.0, rInitial = 0.0;
	};

	static double dot(const double* a, const double* b) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; }
	static bool finite3(const double* a) { return std::isfinite(a[0]) && std::isfinite(a[1]) && std::isfinite(a[2]); }
	static double maxAbs(const double* a) { return std::fmax(std::fmax(std::fabs(a[0]), std::fabs(a[1])), std::fabs(a[2])); }
	static void stop(Win& s, int status)
	{
		s.phase = kDone;
		s.status = status;
	}

	// N2
	void trial(Win& s) const
	{
		s.slope = -dot(s.gf, s.gf);
		for (int k = 0; k < 3; ++k)
		{
			const double d = -s.gf[k];
			s.trial[k] = s.om[k] + s.alpha * d;
		}
		s.phase = kTrial;
	}

	void step(Win& s, double r, const double* g)
	{
		const double ft = -r;
		const double gt[3] = {-g[0], -g[1], -g[2]};
		s.evaluations += 1;
		if (s.phase == kFirst)
		{
			// N1
			s.rInitial = r;
			s.f = ft;
			for (int k = 0; k < 3; ++k)
			{
				s.gf[k] = gt[k];
			}
			if (!(std::isfinite(ft) && finite3(gt)))
			{
				return stop(s, EBO_ROT_NONFINITE);
			}
			const double gmax = maxAbs(gt);
			if (gmax == 0.0)
			{
				return stop(s, EBO_ROT_CONVERGED_GRADIENT);
			}
			s.alpha = o_.first_rate / gmax;
			return trial(s);
		}
		// N3
		const bool accepted = std::isfinite(ft) && finite3(gt) && ft <= s.f + (o_.c1 * s.alpha) * s.slope;
		if (!accepted)
		{
			s.alpha = s.alpha / 2.0;
			s.backtracks += 1;
			if (s.backtracks >= o_.max_backtracks)
			{
				return stop(s, EBO_ROT_NO_PROGRESS);
			}
			return trial(s);
		}
		// N4
		double sv[3], yv[3];
		for (int k = 0; k < 3; ++k)
		{
			sv[k] = s.trial[k] - s.om[k];
			yv[k] = gt[k] - s.gf[k];
			s.om[k] = s.trial[k];
			s.gf[k] = gt[k];
		}
		s.f = ft;
		s.iterations += 1;
		s.backtracks = 0;
		if (maxAbs(sv) < o_.step_tol)
		{
			return stop(s, EBO_ROT_CONVERGED_STEP);
		}
		if (s.iterations == o_.max_iterations)
		{
			return stop(s, EBO_ROT_MAX_ITERATIONS);
		}
		const double sy = dot(sv, yv);
		s.alpha = sy > 0.0 ? dot(sv, sv) / sy : 2.0 * s.alpha;
		trial(s);
	}

	ebo_rot_solver_opts o_;
	std::vector<Win> w_;
};
}  // namespace ebo
