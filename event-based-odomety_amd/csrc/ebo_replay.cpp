// ebo_replay.cpp — replaying a recording window by window (include/ebo.h, "recordings"): the reference's window rule
// on a time-ordered stream (ebo_cut_windows, host only) and R2 + R3 for many windows in lock-step chunks
// (ebo_compensate_windows).  No kernel of its own: a chunk is ebo_set_windows, ebo_solve and two ebo_count_image calls.
#include "ebo_ctx.h"

using namespace ebo;

extern "C" {

// tools::Evaluator::eventCallback (evaluator.cpp:32-45) after FeatureDetector::addEvent (feature_detector.cpp:621-628):
// push the event, pop the front while more than max_store are held, THEN test
//   (ts - lastCompensation).count() >= time  ||  size >= count
// and on a trigger hand the held events (the triggering one last) to the compensation, lastCompensation = ts.
int ebo_cut_windows(const ebo_event* ev, size_t n, int64_t last_compensation_us, uint32_t time_us, uint32_t count,
					uint64_t max_store, size_t* begin, size_t* end, size_t cap, size_t* n_windows,
					int64_t* last_compensation_out, size_t* pending_begin)
{
	if ((!ev && n) || !n_windows || !last_compensation_out || !pending_begin || (cap && (!begin || !end)) ||
		max_store == 0)
	{
		return EBO_ERR_ARG;
	}
	size_t start = 0, nw = 0;
	int64_t last = last_compensation_us;
	for (size_t i = 0; i < n; ++i)
	{
		if (i + 1 - start > max_store)
		{
			start = i + 1 - max_store;
		}
		const size_t held = i + 1 - start;
		if (ev[i].t_us - last >= static_cast<int64_t>(time_us) || held >= count)
		{
			if (nw < cap)
			{
				begin[nw] = start;
				end[nw] = i + 1;
			}
			++nw;
			last = ev[i].t_us;
			start = i + 1;
		}
	}
	*n_windows = nw;
	if (nw > cap)
	{
		return EBO_ERR_RANGE;
	}
	*last_compensation_out = last;
	*pending_begin = start;
	return EBO_OK;
}

// One chunk: the windows `ids` (in order), whose events are base[off[k] .. off[k+1]).  On success every output
// of the chunk is written at its window's place and status[id] = EBO_OK.
namespace
{
struct Outputs
{
	const ebo_solver_opts* o;
	double* flows;
	double* warped;
	double* integrated;
	ebo_summary* summary;
	int32_t* status;
};

int run_chunk(ebo_ctx* c, const ebo_event* base, const std::vector<size_t>& off, const std::vector<int>& ids,
			  const Outputs& out)
{
	const int k = static_cast<int>(ids.size());
	int rc = ebo_set_windows(c, base, off.data(), k);
	if (rc)
	{
		return rc;
	}
	const size_t P = static_cast<size_t>(c->P), npix = static_cast<size_t>(c->prm.image_w) * c->prm.image_h;
	// the normal case writes straight into the caller's arrays; a chunk that lost a window in the middle
	// (error path only) goes through scratch and is scattered afterwards
	bool contiguous = true;
	for (int j = 1; j < k; ++j)
	{
		contiguous = contiguous && ids[j] == ids[j - 1] + 1;
	}
	std::vector<double> sFlows, sWarped, sIntegrated;
	std::vector<ebo_summary> sSumm(k);
	double* flows = out.flows + static_cast<size_t>(ids[0]) * P * 2;
	double* warped = out.warped ? out.warped + static_cast<size_t>(ids[0]) * npix : nullptr;
	double* integrated = out.integrated ? out.integrated + static_cast<size_t>(ids[0]) * npix : nullptr;
	if (!contiguous)
	{
		sFlows.resize(static_cast<size_t>(k) * P * 2);
		flows = sFlows.data();
		if (warped)
		{
			sWarped.resize(static_cast<size_t>(k) * npix);
			warped = sWarped.data();
		}
		if (integrated)
		{
			sIntegrated.resize(static_cast<size_t>(k) * npix);
			integrated = sIntegrated.data();
		}
	}
	rc = ebo_solve(c, out.o, flows, sSumm.data());
	if (!rc && warped)
	{
		rc = ebo_count_image(c, EBO_COUNT_WARPED, flows, warped);
	}
	if (!rc && integrated)
	{
		rc = ebo_count_image(c, EBO_COUNT_INTEGRATED, nullptr, integrated);
	}
	if (rc)
	{
		return rc;
	}
	for (int j = 0; j < k; ++j)
	{
		const size_t w = static_cast<size_t>(ids[j]);
		if (!contiguous)
		{
			std::memcpy(out.flows + w * P * 2, flows + j * P * 2, P * 2 * sizeof(double));
			if (warped)
			{
				std::memcpy(out.warped + w * npix, warped + j * npix, npix * sizeof(double));
			}
			if (integrated)
			{
				std::memcpy(out.integrated + w * npix, integrated + j * npix, npix * sizeof(double));
			}
		}
		if (out.summary)
		{
			out.summary[w] = sSumm[j];
		}
		out.status[w] = EBO_OK;
	}
	return EBO_OK;
}
}  // namespace

int ebo_compensate_windows(ebo_ctx* c, const ebo_event* ev, const size_t* offsets, int n_windows,
						   const ebo_solver_opts* o, double* flows_out, double* warped_out, double* integrated_out,
						   ebo_summary* summary, int32_t* status)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!offsets || n_windows <= 0 || !flows_out || (!ev && offsets[n_windows] > offsets[0]))
	{
		return c->fail(EBO_ERR_ARG, "null events/offsets/flows or no window");
	}
	for (int w = 0; w < n_windows; ++w)
	{
		if (offsets[w + 1] < offsets[w])
		{
			return c->fail(EBO_ERR_ARG, "offsets must be non-decreasing");
		}
	}
	int rc = ebo_host::check_solver_opts(c, o);
	if (rc)
	{
		return rc;
	}
	std::vector<int32_t> ownStatus;
	if (!status)
	{
		ownStatus.resize(n_windows);
		status = ownStatus.data();
	}
	const Outputs out{o, flows_out, warped_out, integrated_out, summary, status};
	int firstBad = -1;
	std::string firstMsg;
	auto refuse = [&](int w, int code, const std::string& msg) {
		status[w] = code;
		if (firstBad < 0 || w < firstBad)
		{
			firstBad = w;
			firstMsg = msg;
		}
	};
	std::vector<ebo_event> staging;
	std::vector<size_t> off;
	std::vector<int> ids;
	int w = 0;
	while (w < n_windows)
	{
		// the chunk: as many following windows as max_windows / max_events admit (at least one)
		ids.clear();
		size_t events = 0;
		for (; w < n_windows && static_cast<int>(ids.size()) < c->cap_windows; ++w)
		{
			const size_t nw = offsets[w + 1] - offsets[w];
			if (nw == 0)
			{
				refuse(w, EBO_ERR_ARG, "empty window");  // as ebo_compensate_events_contrast
				continue;
			}
			if (!ids.empty() && events + nw > c->cap_events)
			{
				break;
			}
			ids.push_back(w);
			events += nw;
		}
		if (ids.empty())
		{
			continue;
		}
		// empty windows are zero-length, so the chunk's windows are adjacent in ev
		off.assign(ids.size() + 1, 0);
		for (size_t j = 0; j < ids.size(); ++j)
		{
			off[j] = offsets[ids[j]];
		}
		off[ids.size()] = offsets[ids.back() + 1];
		rc = run_chunk(c, ev, off, ids, out);
		if (rc == EBO_ERR_RANGE || rc == EBO_ERR_ARG)
		{
			// error path: the loader refused the chunk (its range checks partly run on the device).  Find the
			// windows it refuses alone, then reload the chunk without them.
			std::vector<int> keep;
			for (int id : ids)
			{
				const int r1 = ebo_set_window(c, ev + offsets[id], offsets[id + 1] - offsets[id]);
				if (r1)
				{
					refuse(id, r1, c->err);
				}
				else
				{
					keep.push_back(id);
				}
			}
			ids.swap(keep);
			if (ids.empty())
			{
				continue;
			}
			staging.clear();
			off.assign(1, 0);
			for (int id : ids)
			{
				staging.insert(staging.end(), ev + offsets[id], ev + offsets[id + 1]);
				off.push_back(staging.size());
			}
			rc = run_chunk(c, staging.data(), off, ids, out);
		}
		if (rc)
		{
			for (int id : ids)
			{
				refuse(id, rc, c->err);
			}
		}
	}
	if (firstBad >= 0)
	{
		return c->fail(status[firstBad], "window " + std::to_string(firstBad) + ": " + firstMsg);
	}
	return EBO_OK;
}

}  // extern "C"
