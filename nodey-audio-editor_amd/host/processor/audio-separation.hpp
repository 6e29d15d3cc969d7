// processor/audio-separation.hpp — a node the reference has no class for: harmonic/percussive separation by medians over the library's STFT
// (nae_hpss_*; DESIGN.md §3, "K21 separation").  Registered by infra::register_separation_processors().  Its process_payload stands in
// audio-effects.cpp, on the loop the handle nodes share (run_on_handle).
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_separation": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "harmonic_db"    -120 ... 12: the level of the tonal part; -120 removes it                   (default 0)
	//   "percussive_db"  -120 ... 12: the level of the transient part; -120 removes it              (default -120: the node removes the transients)
	//   "mask"           "soft" | "hard": a bin is shared between the parts by their medians' ratio,
	//                    or goes whole to the larger one                                            (default "soft")
	//   "fft_size"       512 | 1024 | 2048 | 4096                                                  (default 2048)
	//   "time_span"      integer 0 ... 8: frames to either side of the harmonic median               (default 8)
	//   "freq_span"      integer 0 ... 8: bins to either side of the percussive median               (default 8)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  A user who wants
	// both parts runs two nodes.  The node delivers exactly the frames it received, as packed float frames of their sizes, pts and time base,
	// and flushes at the end of the stream.
	// the keys above as a plain copyable record: the node is one
	struct Separation_settings
	{
		enum class Mask { Soft, Hard };
		static constexpr double default_harmonic_db = 0, default_percussive_db = -120;
		static constexpr int default_fft_size = 2048, default_time_span = 8, default_freq_span = 8;
		double harmonic_db = default_harmonic_db, percussive_db = default_percussive_db;
		Mask mask = Mask::Soft;
		int fft_size = default_fft_size, time_span = default_time_span, freq_span = default_freq_span;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_separation : public infra::Processor, public Separation_settings
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
