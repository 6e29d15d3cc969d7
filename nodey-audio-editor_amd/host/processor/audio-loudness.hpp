// processor/audio-loudness.hpp — a node the reference has no class for: loudness normalization to a delivery level by the library's BS.1770
// meter (nae_loud_*; DESIGN.md §3, "K14 loudness").  Registered by infra::register_mastering_processors().  Its process_payload stands in
// audio-effects.cpp.
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Registered as "audio_loudness": one audio input pin, one audio output pin.  JSON keys, all optional:
	//   "target_lufs"   -70 ... -5: the integrated loudness the stream is brought to     (default -14)
	//   "true_peak_db"  -20 ... 0: the true-peak ceiling in dBTP the gain must respect   (default -1)
	//   "max_gain_db"   0 ... 40: the most the node turns a stream up                     (default 20)
	// A value of the wrong type or outside these ranges: Runtime_error "Wrong field: <key>".  Defaults are not written back.  The gain is one
	// number for the whole stream and is known only at its end: the node feeds a measuring handle (nae_loud) as the frames arrive and holds
	// their samples in host memory as interleaved f32 — 8 bytes per stereo sample frame, 23 MB per minute at 48 kHz — until the stream ends.  It
	// then delivers exactly the frames it received, as packed float frames of their sizes, pts and time base, every sample times the one gain:
	// the bits of nae_loud_normalize_f32 on the whole stream.  A stream shorter than 400 ms has no gating block and no loudness: its frames pass
	// as they are, and no GPU is touched.  A sample rate outside 8000 ... 192000 or not a multiple of 10 is a Runtime_error once 400 ms arrived; a frame of another rate than the first's
	// is one at once.
	// the keys above as a plain copyable record: the node is one
	struct Loudness_settings
	{
		static constexpr double default_target_lufs = -14, default_true_peak_db = -1, default_max_gain_db = 20;
		double target_lufs = default_target_lufs, true_peak_db = default_true_peak_db, max_gain_db = default_max_gain_db;

		void clamp();   // what the widgets would keep; the fields are stated once, in audio-effects.cpp (node-fields.hpp)
	};

	class Audio_loudness : public infra::Processor, public Loudness_settings
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
