// processor/audio-denoise.hpp — a node the reference has no class for: noise reduction by a spectral gate on the library's STFT
// (nae_denoise_*; DESIGN.md §3, "K13 spectral gate").  Registered by infra::register_restoration_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop that feeds a streaming handle and delivers its frames.
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_denoise": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "reduction_db"      0 ... 48: how far a bin judged to be noise is turned down              (default 12)
	//   "sensitivity_db"    -6 ... 24: how far above the learned noise power a bin must stand       (default 6)
	//   "fft_size"          512 | 1024 | 2048 | 4096                                               (default 2048)
	//   "time_smooth"       integer 0 ... 8: frames the decisions are smoothed over, to either side  (default 2)
	//   "freq_smooth"       integer 0 ... 4: bins they are smoothed over, to either side             (default 2)
	//   "profile_start_ms"  0 ... 60000: where the stretch of noise the node learns from begins      (default 0)
	//   "profile_ms"        20 ... 10000: its length                                                (default 500)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  The node learns
	// the noise from the stretch [profile_start_ms, profile_start_ms + profile_ms) of its own input: it holds the frames until that stretch
	// has arrived or the stream ends, computes one profile per channel on the device (nae_denoise_profile_f32) and then runs everything it held
	// and the rest through the gate.  A stream that ends with fewer than fft_size samples in the stretch is a Runtime_error.  The node delivers
	// exactly the frames it received, as packed float frames of their sizes, pts and time base, and flushes at the end of the stream.
	// the keys above as a plain copyable record: the node is one
	struct Denoise_settings
	{
		static constexpr double default_reduction_db = 12, default_sensitivity_db = 6, default_profile_start_ms = 0, default_profile_ms = 500;
		static constexpr int default_fft_size = 2048, default_time_smooth = 2, default_freq_smooth = 2;
		double reduction_db = default_reduction_db, sensitivity_db = default_sensitivity_db, profile_start_ms = default_profile_start_ms,
			   profile_ms = default_profile_ms;
		int fft_size = default_fft_size, time_smooth = default_time_smooth, freq_smooth = default_freq_smooth;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_denoise : public infra::Processor, public Denoise_settings
	{
	  public:

		static infra::Processor::Info get_processor_info();
		Processor::Info get_processor_info_non_static() const override { return get_processor_info(); }
		void draw_title() override;                         // bodies: draw-headless.cpp
		bool draw_content(bool readonly) override;
		std::vector<infra::Processor::Pin_attribute> get_pin_attributes() const override;
		void process_payload(
			const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
			const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
			const std::atomic<bool>& stop_token,
			std::any& user_data
		) override;
		Json::Value serialize() const override;
		void deserialize(const Json::Value& value) override;
	};
}
