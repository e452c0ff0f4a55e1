// ebo_trackerr.cpp — the track-evaluation entry points of include/ebo.h (V1-V9): where KLT reference tracks start
// (ebo_track_seeds, host), the reference tracks themselves as the loop over ebo_lk_add_image / ebo_lk_track that
// defines them (ebo_reference_tracks), the errors and ages of many (track, threshold) units in one launch, one wave
// per unit (ebo_track_errors; the kernel is in ebo_trackerr.inc), and the two figures of the report over one threshold
// (ebo_track_error_summary, host).
#include "ebo_ctx.h"

#include <chrono>
#include <cmath>
#include <vector>

using namespace ebo;

namespace
{
// offsets of n groups: start at 0, do not decrease, no group beyond the limit
bool offsetsOk(const int* off, int n)
{
	if (off[0] != 0)
	{
		return false;
	}
	for (int k = 0; k < n; ++k)
	{
		if (off[k + 1] < off[k] || off[k + 1] - off[k] > kTeMaxTrackSamples)
		{
			return false;
		}
	}
	return true;
}

// times within every group: non-decreasing, or strictly increasing
bool timesOk(const int* off, int n, const int64_t* t, bool strictly)
{
	for (int k = 0; k < n; ++k)
	{
		for (int i = off[k] + 1; i < off[k + 1]; ++i)
		{
			if (t[i] < t[i - 1] || (strictly && t[i] == t[i - 1]))
			{
				return false;
			}
		}
	}
	return true;
}

int trackErrors(ebo_ctx* c, int n, const int* estOff, const int64_t* estT, const double* estXy, const int* gtOff, const int64_t* gtT,
				const double* gtXy, int nTaus, const double* taus, bool hostArrays, ebo_track_error_result* results, double* sampleErr)
{
	int rc = enter(c, "ebo_track_errors: a track count outside [0, 65535] or a threshold count outside [0, 8]",
				   n >= 0 && n <= kTeMaxTracks && nTaus >= 0 && nTaus <= kTeMaxTaus);
	if (rc)
	{
		return rc;
	}
	auto bad = [&](const char* what) { return c->fail(EBO_ERR_ARG, std::string("ebo_track_errors: ") + what); };
	if (n > 0 && (!estOff || !gtOff))
	{
		return bad("null offsets");
	}
	if (nTaus > 0 && !taus)
	{
		return bad("null taus");
	}
	if (n > 0 && (!offsetsOk(estOff, n) || !offsetsOk(gtOff, n)))
	{
		return bad("offsets that decrease or do not start at 0, or a track beyond 2^24 samples");
	}
	for (int j = 0; j < nTaus; ++j)
	{
		if (!(taus[j] >= 0.0))
		{
			return bad("a tau that is NaN or negative");
		}
	}
	if (n == 0 || nTaus == 0)
	{
		return EBO_OK;
	}
	if (!results)
	{
		return bad("null results");
	}
	const int nEst = estOff[n], nGt = gtOff[n];
	if ((nEst > 0 && (!estT || !estXy)) || (nGt > 0 && (!gtT || !gtXy)))
	{
		return bad("null samples");
	}
	if (hostArrays && !timesOk(estOff, n, estT, false))
	{
		return bad("estimated times that decrease within a track");
	}
	if (hostArrays && !timesOk(gtOff, n, gtT, true))
	{
		return bad("ground-truth times that do not increase strictly within a track");
	}
	const auto wall0 = std::chrono::steady_clock::now();
	const size_t units = static_cast<size_t>(n) * static_cast<size_t>(nTaus);
	const size_t bOff = (static_cast<size_t>(n) + 1) * sizeof(int), bTaus = static_cast<size_t>(nTaus) * sizeof(double);
	const size_t bEstT = static_cast<size_t>(nEst) * sizeof(int64_t), bEstXy = 2 * static_cast<size_t>(nEst) * sizeof(double);
	const size_t bGtT = static_cast<size_t>(nGt) * sizeof(int64_t), bGtXy = 2 * static_cast<size_t>(nGt) * sizeof(double);
	const size_t bErr = static_cast<size_t>(nEst) * sizeof(double);
	ScratchCarve cv;
	const size_t oEstOff = cv.take(bOff), oGtOff = cv.take(bOff), oTaus = cv.take(bTaus);
	const size_t oRes = cv.take(units * sizeof(ebo_track_error_result));
	size_t oEstT = 0, oEstXy = 0, oGtT = 0, oGtXy = 0, oErr = 0;
	if (hostArrays)
	{
		oEstT = cv.take(bEstT);
		oEstXy = cv.take(bEstXy);
		oGtT = cv.take(bGtT);
		oGtXy = cv.take(bGtXy);
		oErr = cv.take(sampleErr ? bErr : 0);
	}
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipSuccess;
	auto up = [&](size_t off, const void* src, size_t bytes) {
		if (e == hipSuccess && bytes)
		{
			e = hipMemcpyAsync(c->scratch<char>(off), src, bytes, hipMemcpyHostToDevice, c->stream);
		}
	};
	up(oEstOff, estOff, bOff);
	up(oGtOff, gtOff, bOff);
	up(oTaus, taus, bTaus);
	const int64_t* dEstT = estT;
	const double* dEstXy = estXy;
	const int64_t* dGtT = gtT;
	const double* dGtXy = gtXy;
	double* dErr = sampleErr;
	if (hostArrays)
	{
		up(oEstT, estT, bEstT);
		up(oEstXy, estXy, bEstXy);
		up(oGtT, gtT, bGtT);
		up(oGtXy, gtXy, bGtXy);
		dEstT = c->scratch<int64_t>(oEstT);
		dEstXy = c->scratch<double>(oEstXy);
		dGtT = c->scratch<int64_t>(oGtT);
		dGtXy = c->scratch<double>(oGtXy);
		dErr = sampleErr ? c->scratch<double>(oErr) : nullptr;
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "track error uploads");
	}
	mark(c, 0);
	if (launch_track_errors(nEst, nGt, n, c->scratch<int>(oEstOff), dEstT, dEstXy, c->scratch<int>(oGtOff), dGtT, dGtXy, nTaus,
							c->scratch<double>(oTaus), c->scratch<ebo_track_error_result>(oRes), dErr, c->stream))
	{
		return c->hip(hipGetLastError(), "track error kernel launch");
	}
	mark(c, 1);
	e = hipMemcpyAsync(results, c->scratch<char>(oRes), units * sizeof(ebo_track_error_result), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess && hostArrays && sampleErr && bErr)
	{
		e = hipMemcpyAsync(sampleErr, dErr, bErr, hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "track error results");
	}
	if (c->tv_timing)
	{
		// slot 0: the kernel; slot 4: the whole call (wall clock); the others do not apply
		(void)hipEventElapsedTime(&c->tv_ms[0], c->tv_ev[0], c->tv_ev[1]);
		c->tv_ms[1] = c->tv_ms[2] = c->tv_ms[3] = 0.0f;
		c->tv_ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
	}
	return EBO_OK;
}
}  // namespace

extern "C" {

void ebo_default_lk_params(ebo_lk_params* p)
{
	if (p)
	{
		// FlowEstimator's values (flow_estimator.cpp:86-108)
		p->win_w = p->win_h = 21;
		p->max_level = 3;
		p->max_count = 30;
		p->epsilon = 0.01;
		p->min_eig_threshold = 1e-4;
	}
}

int ebo_track_seeds(int n_tracks, const int* est_off, const int64_t* est_t_us, const double* est_xy, int n_frames,
					const int64_t* frame_t_us, int* seed_frame, float* seed_xy)
{
	if (n_tracks < 0 || n_frames < 0 || (n_tracks > 0 && (!est_off || !seed_frame || !seed_xy)) || (n_frames > 0 && !frame_t_us))
	{
		return EBO_ERR_ARG;
	}
	if (n_tracks == 0)
	{
		return EBO_OK;
	}
	if (!offsetsOk(est_off, n_tracks) || (est_off[n_tracks] > 0 && (!est_t_us || !est_xy)) || !timesOk(est_off, n_tracks, est_t_us, false))
	{
		return EBO_ERR_ARG;
	}
	for (int f = 1; f < n_frames; ++f)
	{
		if (frame_t_us[f] <= frame_t_us[f - 1])
		{
			return EBO_ERR_ARG;
		}
	}
	for (int k = 0; k < n_tracks; ++k)
	{
		const int b = est_off[k], n = est_off[k + 1] - b;
		seed_frame[k] = -1;
		seed_xy[2 * k] = seed_xy[2 * k + 1] = 0.0f;
		if (n == 0)
		{
			continue;
		}
		const int64_t* t = est_t_us + b;
		// the first frame at or after the track's first sample
		int lo = 0, hi = n_frames;
		while (lo < hi)
		{
			const int mid = lo + (hi - lo) / 2;
			if (frame_t_us[mid] < t[0])
			{
				lo = mid + 1;
			}
			else
			{
				hi = mid;
			}
		}
		if (lo == n_frames || frame_t_us[lo] > t[n - 1])
		{
			continue;
		}
		const int64_t T = frame_t_us[lo];
		double gx, gy;
		te_interp(t, est_xy + 2 * static_cast<size_t>(b), n, te_search(t, n, te_steps(n), T), T, gx, gy);
		seed_frame[k] = lo;
		seed_xy[2 * k] = static_cast<float>(gx);
		seed_xy[2 * k + 1] = static_cast<float>(gy);
	}
	return EBO_OK;
}

int ebo_reference_tracks(ebo_ctx* c, int n_frames, const uint8_t* frames, const int64_t* frame_t_us, int n, const int* seed_frame,
						 const float* seed_xy, const ebo_lk_params* lk_or_null, int* first, int* last, double* xy)
{
	int rc = enter(c, "ebo_reference_tracks: negative counts or a needed pointer that is null",
				   n_frames >= 0 && n >= 0 && (n_frames == 0 || (frames && frame_t_us)) &&
					   (n == 0 || (seed_frame && seed_xy && first && last && (xy || n_frames == 0))));
	if (rc)
	{
		return rc;
	}
	for (int k = 0; k < n; ++k)
	{
		if (seed_frame[k] >= n_frames)
		{
			return c->fail(EBO_ERR_ARG, "ebo_reference_tracks: a seed frame beyond the frames");
		}
	}
	ebo_lk_params lk;
	ebo_default_lk_params(&lk);
	if (lk_or_null)
	{
		lk = *lk_or_null;
	}
	const int w = c->prm.image_w, h = c->prm.image_h;
	const size_t frameBytes = static_cast<size_t>(w) * static_cast<size_t>(h);
	for (int k = 0; k < n; ++k)
	{
		first[k] = last[k] = seed_frame[k] < 0 ? -1 : seed_frame[k];
	}
	std::fill(xy, xy + 2 * static_cast<size_t>(n) * static_cast<size_t>(n_frames), 0.0);
	auto at = [&](int k, int f) { return xy + 2 * (static_cast<size_t>(k) * static_cast<size_t>(n_frames) + static_cast<size_t>(f)); };
	std::vector<char> alive(static_cast<size_t>(n), 0);
	std::vector<int> who;
	std::vector<float> prev, next;
	std::vector<uint8_t> status;
	if (n_frames > 0)
	{
		rc = ebo_lk_add_image(c, frames);
		if (rc)
		{
			return rc;
		}
	}
	for (int f = 0; f < n_frames; ++f)
	{
		for (int k = 0; k < n; ++k)
		{
			if (seed_frame[k] == f)
			{
				alive[k] = 1;
				at(k, f)[0] = static_cast<double>(seed_xy[2 * k]);
				at(k, f)[1] = static_cast<double>(seed_xy[2 * k + 1]);
			}
		}
		if (f + 1 == n_frames)
		{
			break;
		}
		rc = ebo_lk_add_image(c, frames + frameBytes * static_cast<size_t>(f + 1));
		if (rc)
		{
			return rc;
		}
		who.clear();
		prev.clear();
		for (int k = 0; k < n; ++k)
		{
			if (alive[k])
			{
				who.push_back(k);
				prev.push_back(static_cast<float>(at(k, f)[0]));
				prev.push_back(static_cast<float>(at(k, f)[1]));
			}
		}
		if (who.empty())
		{
			continue;
		}
		next.assign(prev.size(), 0.0f);
		status.assign(who.size(), 0);
		rc = ebo_lk_track(c, static_cast<int>(who.size()), prev.data(), next.data(), status.data(), nullptr, lk.win_w, lk.win_h,
						  lk.max_level, lk.max_count, lk.epsilon, lk.min_eig_threshold);
		if (rc)
		{
			return rc;
		}
		for (size_t i = 0; i < who.size(); ++i)
		{
			const int k = who[i];
			const float x = next[2 * i], y = next[2 * i + 1];
			if (status[i] == 1 && x >= 0.0f && x < static_cast<float>(w) && y >= 0.0f && y < static_cast<float>(h))
			{
				at(k, f + 1)[0] = static_cast<double>(x);
				at(k, f + 1)[1] = static_cast<double>(y);
				last[k] = f + 1;
			}
			else
			{
				alive[k] = 0;
			}
		}
	}
	return EBO_OK;
}

int ebo_track_errors(ebo_ctx* c, int n_tracks, const int* est_off, const int64_t* est_t_us, const double* est_xy, const int* gt_off,
					 const int64_t* gt_t_us, const double* gt_xy, int n_taus, const double* taus, ebo_track_error_result* results,
					 double* sample_err_out_or_null)
{
	return trackErrors(c, n_tracks, est_off, est_t_us, est_xy, gt_off, gt_t_us, gt_xy, n_taus, taus, true, results,
					   sample_err_out_or_null);
}

int ebo_track_errors_device(ebo_ctx* c, int n_tracks, const int* est_off, const int64_t* d_est_t_us, const double* d_est_xy,
							const int* gt_off, const int64_t* d_gt_t_us, const double* d_gt_xy, int n_taus, const double* taus,
							ebo_track_error_result* results, double* d_sample_err_out_or_null)
{
	return trackErrors(c, n_tracks, est_off, d_est_t_us, d_est_xy, gt_off, d_gt_t_us, d_gt_xy, n_taus, taus, false, results,
					   d_sample_err_out_or_null);
}

int ebo_track_error_summary(int n_tracks, const ebo_track_error_result* results, int stride, ebo_track_error_summary_result* out)
{
	if (!out || n_tracks < 0 || stride < 1 || (n_tracks > 0 && !results))
	{
		return EBO_ERR_ARG;
	}
	double sumErr = 0.0, sumAge = 0.0;
	int m = 0, outlived = 0;
	for (int k = 0; k < n_tracks; ++k)
	{
		const ebo_track_error_result& r = results[static_cast<size_t>(k) * static_cast<size_t>(stride)];
		if (r.status == 0 && r.n_inliers >= 1)
		{
			sumErr = sumErr + r.err_mean;
			sumAge = sumAge + static_cast<double>(r.age_us);
			outlived += r.cut == -1 ? 1 : 0;
			++m;
		}
	}
	out->mean_error = m ? sumErr / static_cast<double>(m) : 0.0;
	out->mean_age_s = m ? (sumAge / static_cast<double>(m)) * 1e-6 : 0.0;
	out->counted = m;
	out->discarded = m ? n_tracks - m : 0;
	out->outlived = outlived;
	out->pad = 0;
	return EBO_OK;
}

}  // extern "C"
