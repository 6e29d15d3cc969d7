// processor/draw-headless.cpp — the two GUI hooks of every GPU processor, without a GUI.
//
// In the reference draw_title() / draw_content(bool readonly) are pure virtual (/root/reference/include/infra/processor.hpp:99-104), run on the
// GUI thread once per displayed frame (src/frontend/app.cpp:264-265), and are the ONLY code that changes a node's parameters while the editor
// runs: `volume` is not even serialised (include/processor/audio-vol.hpp:57-58; slider and clamp: src/processor/audio-vol.cpp:257-281), the
// mixer's weights are renormalised there so that the unlocked ones sum to 1 (audio-amix.cpp:331-393), `bias` (audio-bimix.cpp:338-356),
// `velocity` / `keep_pitch` (audio-velocity.cpp:107-133) and `pitch` (:135-149) have no other writer besides deserialize().
//
// An integrator therefore does NOT link this file: the reference's own bodies of these functions (ImGui calls around the same member names —
// volume, input_num / volumes / locks, bias, velocity / keep_pitch, pitch) compile unchanged as members of the GPU classes and take its place.
// What stands here is what those bodies do to the parameters when no widget is touched — the clamps and the mixer's renormalisation — so that a
// headless host (tests/host/selftest, an export tool) that calls draw_content() once after editing parameters gets the values the editor
// would run with.  Every body returns what the reference returns when nothing changed: false (true = "pins changed", audio-amix.cpp:344-348).
#include <algorithm>

#include "audio-filter.hpp"
#include "audio-reverb.hpp"
#include "audio-eq.hpp"
#include "audio-dynamics.hpp"
#include "audio-sidechain.hpp"
#include "audio-echo.hpp"
#include "audio-modulation.hpp"
#include "audio-saturation.hpp"
#include "audio-gate.hpp"
#include "audio-denoise.hpp"
#include "audio-loudness.hpp"
#include "audio-mix.hpp"
#include "audio-velocity.hpp"
#include "audio-vol.hpp"
#include "nae_dsp_spec.h"

namespace processor
{
	void Audio_vol::draw_title() {}
	bool Audio_vol::draw_content(bool)
	{
		set_volume(volume);  // [0, max_volume = 10]
		return false;
	}

	void Audio_amix::draw_title() {}
	bool Audio_amix::draw_content(bool)
	{
		input_num = std::clamp(input_num, 1, 16);
		volumes.resize(input_num, 1.0f);
		locks.resize(input_num, false);
		float unlocked = 0.0f;
		for (int i = 0; i < input_num; i++) unlocked += locks[i] ? 0.0f : volumes[i];
		unlocked = std::max(unlocked, 0.001f);
		for (int i = 0; i < input_num; i++)
			if (!locks[i]) volumes[i] /= unlocked;
		return false;
	}

	void Audio_bimix::draw_title() {}
	bool Audio_bimix::draw_content(bool)
	{
		bias = std::clamp(bias, -1.0f, 1.0f);
		return false;
	}

	void Audio_bimix_v2::draw_title() {}
	bool Audio_bimix_v2::draw_content(bool) { return false; }

	void Velocity_modifier::draw_title() {}
	bool Velocity_modifier::draw_content(bool)
	{
		velocity = std::clamp(velocity, 0.5f, 3.0f);  // ImGuiSliderFlags_AlwaysClamp
		return false;
	}

	void Pitch_modifier::draw_title() {}
	bool Pitch_modifier::draw_content(bool) { return false; }

	void Audio_spectrum::draw_title() {}
	bool Audio_spectrum::draw_content(bool) { return false; }

	void Audio_filter::draw_title() {}
	bool Audio_filter::draw_content(bool)
	{
		// what the widgets would keep: an odd tap count in range, corners in order, and a frame size the taps fit (else the library's pick)
		taps = std::clamp(taps, 1, max_taps) | 1;
		f_lo = std::max(f_lo, 1.0f);
		f_hi = std::max(f_hi, 1.0f);
		if ((kind == Kind::Bandpass || kind == Kind::Bandstop) && f_lo > f_hi) std::swap(f_lo, f_hi);
		if (fft_size != 0 && taps > fft_size / 2 + 1) fft_size = 0;
		return false;
	}

	void Audio_reverb::draw_title() {}
	bool Audio_reverb::draw_content(bool)
	{
		// what the widgets would keep: every value inside its range
		rt60 = std::clamp(rt60, 0.1, 5.0);
		predelay_ms = std::clamp(predelay_ms, 0.0, 200.0);
		wet = std::clamp(wet, 0.0, 1.0);
		dry = std::clamp(dry, 0.0, 1.0);
		return false;
	}

	void Audio_eq::draw_title() {}
	bool Audio_eq::draw_content(bool)
	{
		// what the widgets would keep: at most 16 bands, every value inside its range
		if (bands.size() > max_bands) bands.resize(max_bands);
		for (auto& b : bands)
		{
			b.freq = std::max(b.freq, 1.0);
			b.gain_db = std::clamp(b.gain_db, -24.0, 24.0);
			b.q = std::clamp(b.q, 0.1, 40.0);
		}
		return false;
	}

	void Audio_dynamics::draw_title() {}
	bool Audio_dynamics::draw_content(bool)
	{
		clamp();   // what the widgets would keep: every value inside its range
		return false;
	}

	void Audio_sidechain::draw_title() {}
	bool Audio_sidechain::draw_content(bool)
	{
		// what the widgets would keep: the dynamics' values inside their ranges, at most 4 bands, every band's value inside its range
		dynamics.clamp();
		if (key_filter.size() > max_bands) key_filter.resize(max_bands);
		for (auto& b : key_filter)
		{
			b.freq = std::max(b.freq, 1.0);
			b.gain_db = std::clamp(b.gain_db, -24.0, 24.0);
			b.q = std::clamp(b.q, 0.1, 40.0);
		}
		return false;
	}

	void Audio_echo::draw_title() {}
	bool Audio_echo::draw_content(bool)
	{
		// what the widgets would keep: every value inside its range; a corner between 0 and its lowest value is that value
		delay_ms = std::clamp(delay_ms, 1.0, 1e9);
		if (delay_ms_right.has_value()) delay_ms_right = std::clamp(*delay_ms_right, 1.0, 1e9);
		feedback = std::clamp(feedback, 0.0, 0.95);
		if (damp_hz != 0.0) damp_hz = std::clamp(damp_hz, 200.0, 20000.0);
		if (lowcut_hz != 0.0) lowcut_hz = std::clamp(lowcut_hz, 20.0, 2000.0);
		wet = std::clamp(wet, 0.0, 1.0);
		dry = std::clamp(dry, 0.0, 1.0);
		return false;
	}

	void Audio_modulation::draw_title() {}
	bool Audio_modulation::draw_content(bool)
	{
		// what the widgets would keep: every value inside its range
		rate_hz = std::clamp(rate_hz, 0.0, 20.0);
		delay_ms = std::clamp(delay_ms, 0.05, 1e9);
		depth_ms = std::clamp(depth_ms, 0.0, 1e9);
		feedback = std::clamp(feedback, -0.95, 0.95);
		voices = std::clamp(voices, 1, 4);
		spread = std::clamp(spread, 0.0, 1.0);
		wet = std::clamp(wet, 0.0, 1.0);
		dry = std::clamp(dry, 0.0, 1.0);
		return false;
	}

	void Audio_saturation::draw_title() {}
	bool Audio_saturation::draw_content(bool)
	{
		// what the widgets would keep: every value inside its range, the oversampling factor a power of two
		drive_db = std::clamp(drive_db, 0.0, 48.0);
		bias = std::clamp(bias, 0.0, 1.0);
		oversample = oversample >= 8 ? 8 : oversample >= 4 ? 4 : oversample >= 2 ? 2 : 1;
		output_db = std::clamp(output_db, -24.0, 24.0);
		mix = std::clamp(mix, 0.0, 1.0);
		return false;
	}

	void Audio_gate::draw_title() {}
	bool Audio_gate::draw_content(bool)
	{
		// what the widgets would keep: every value inside its range
		threshold_db = std::clamp(threshold_db, -90.0, 0.0);
		hysteresis_db = std::clamp(hysteresis_db, 0.0, 24.0);
		range_db = std::clamp(range_db, 0.0, 120.0);
		ratio = std::clamp(ratio, 1.0, 100.0);
		attack_ms = std::clamp(attack_ms, 0.0, 500.0);
		hold_ms = std::clamp(hold_ms, 0.0, 10000.0);
		release_ms = std::clamp(release_ms, 1.0, 5000.0);
		lookahead_ms = std::clamp(lookahead_ms, 0.0, 20.0);
		return false;
	}

	void Audio_denoise::draw_title() {}
	bool Audio_denoise::draw_content(bool)
	{
		// what the widgets would keep: every value inside its range, a frame size the library has (else the default)
		reduction_db = std::clamp(reduction_db, 0.0, 48.0);
		sensitivity_db = std::clamp(sensitivity_db, -6.0, 24.0);
		if (fft_size != 512 && fft_size != 1024 && fft_size != 2048 && fft_size != 4096) fft_size = default_fft_size;
		time_smooth = std::clamp(time_smooth, 0, 8);
		freq_smooth = std::clamp(freq_smooth, 0, 4);
		profile_start_ms = std::clamp(profile_start_ms, 0.0, 60000.0);
		profile_ms = std::clamp(profile_ms, 20.0, 10000.0);
		return false;
	}

	void Audio_loudness::draw_title() {}
	bool Audio_loudness::draw_content(bool)
	{
		// what the widgets would keep: every value inside its range
		target_lufs = std::clamp(target_lufs, NAE_LOUD_MIN_TARGET_LUFS, NAE_LOUD_MAX_TARGET_LUFS);
		true_peak_db = std::clamp(true_peak_db, NAE_LOUD_MIN_CEILING_DBTP, 0.0);
		max_gain_db = std::clamp(max_gain_db, 0.0, NAE_LOUD_MAX_GAIN_DB);
		return false;
	}
}
