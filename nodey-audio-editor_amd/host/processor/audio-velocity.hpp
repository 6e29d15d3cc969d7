// processor/audio-velocity.hpp — GPU drop-ins for processor::Velocity_modifier and processor::Pitch_modifier
// (/root/reference/include/processor/audio-velocity.hpp, src/processor/audio-velocity.cpp:265-505), plus the
// FFT spectrum node the reference lists as a feature (README.md:28) but never implemented.
#pragma once
#include "audio-stream.hpp"

namespace processor
{
	// Which GPU implementation stands in for SoundTouch: the phase vocoder BASELINE.json's north_star asks for, or the
	// WSOLA + anti-alias FIR + cubic transposer chain restated from SoundTouch 2.3.2 (nae_wsola_*).
	// A node's JSON may name it ("algorithm": "vocoder" | "soundtouch").  The reference's JSON has no such key
	// (audio-velocity.cpp:479-505), so projects saved by it — and freshly created nodes — get the DEFAULT, which the
	// integrator chooses once at registration: infra::register_all_processors(Stretch_algorithm::Soundtouch) keeps the
	// reference's audible behaviour for saved projects; the plain call (and this library's own default) is the vocoder.
	enum class Stretch_algorithm { Vocoder, Soundtouch };
	const char* algorithm_name(Stretch_algorithm a);
	Stretch_algorithm default_stretch_algorithm();
	void set_default_stretch_algorithm(Stretch_algorithm a);
	Stretch_algorithm algorithm_from_json(const Json::Value& value);
	// "phase_lock" (bool, optional): identity phase locking of the vocoder (NAE_STRETCH_PHASE_LOCK).  No key: false; a value that is not a bool:
	// Runtime_error "Wrong field: phase_lock"; written back only when true.  With "algorithm": "soundtouch" the key is kept and has no effect.
	bool phase_lock_from_json(const Json::Value& value, const char* node_name);
	// "fft_size" (integer, optional): the vocoder's frame size, 512 / 1024 / 2048 / 4096 (nae_stretch_create_n).  No key: 1024; a value that is not
	// one of those, or a size other than 1024 with "phase_lock": true: Runtime_error "Wrong field: fft_size"; written back only when not 1024.
	// With "algorithm": "soundtouch" the key is kept and has no effect.
	int fft_size_from_json(const Json::Value& value, const char* node_name, bool phase_lock);
	// "formant" (bool, optional, Pitch_modifier only): formant-preserving pitch shift (nae_stretch_create_formant, lifter
	// nae_stretch_formant_lifter(sample rate, fft_size)).  No key: false; a value that is not a bool: Runtime_error "Wrong field: formant";
	// written back only when true.  It combines with "phase_lock" and "fft_size"; with "algorithm": "soundtouch" it is kept and has no effect.
	bool formant_from_json(const Json::Value& value, const char* node_name);
	// "formant_shift" (number of semitones, optional, Pitch_modifier only): moves the formants by that much, with or without a pitch change
	// (nae_stretch_create_formant_shift with formant_ratio 2^(semitones / 12) and the default lifter, whether or not "formant" is set; with
	// "pitch": 0 the node then runs the envelope stage instead of being a wire).  No key: 0; a value that is not a number: Runtime_error
	// "Wrong field: formant_shift"; beyond +-24: Runtime_error "Out of range: formant_shift"; written back only when not 0.  It combines with
	// "phase_lock", "fft_size" and "transients"; with "algorithm": "soundtouch" it is kept and has no effect.
	float formant_shift_from_json(const Json::Value& value, const char* node_name);
	// "transients" (bool, optional): transient preservation of the vocoder (NAE_STRETCH_TRANSIENTS: an onset frame resets the synthesis phase).
	// No key: false; a value that is not a bool: Runtime_error "Wrong field: transients"; written back only when true.  It combines with
	// "phase_lock", "fft_size" and "formant"; with "algorithm": "soundtouch" it is kept and has no effect.
	bool transients_from_json(const Json::Value& value, const char* node_name);
	// "link_channels" (bool, optional): channel link of the vocoder (NAE_STRETCH_LINK_CHANNELS: on a stereo stream the onsets of "transients" and
	// the regions of "phase_lock" are decided once per stream, on the two channels' mean power).  No key: false; a value that is not a bool:
	// Runtime_error "Wrong field: link_channels"; written back only when true.  It combines with "phase_lock", "fft_size", "formant",
	// "formant_shift" and "transients"; with "algorithm": "soundtouch" it is kept and has no effect.
	bool link_channels_from_json(const Json::Value& value, const char* node_name);

	class Velocity_modifier : public infra::Processor
	{
		float velocity = 1;
		bool keep_pitch = false;
		Stretch_algorithm algorithm = default_stretch_algorithm();
		bool phase_lock = false;
		int fft_size = 1024;
		bool transients = false;
		bool link_channels = false;

	  public:

		Batch_stats batch_stats;  // of the last process_payload: frames put / waits for their uploads

		static infra::Processor::Info get_processor_info();
		Processor::Info get_processor_info_non_static() const override { return get_processor_info(); }
		void draw_title() override;                         // bodies: draw-headless.cpp (the integrator keeps the reference's ImGui bodies instead)
		bool draw_content(bool readonly) override;
		std::vector<infra::Processor::Pin_attribute> get_pin_attributes() const override;
		void process_payload(
			const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
			const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
			const std::atomic<bool>& stop_token,
			std::any& user_data
		) override;
		Json::Value serialize() const override;            // velocity, keep_pitch (audio-velocity.cpp:479-485); algorithm, phase_lock, fft_size, transients, link_channels when not the default
		void deserialize(const Json::Value& value) override;  // :487-493
	};

	class Pitch_modifier : public infra::Processor
	{
		float pitch = 0;  // semitones
		Stretch_algorithm algorithm = default_stretch_algorithm();
		bool phase_lock = false;
		int fft_size = 1024;
		bool formant = false;
		float formant_shift = 0;  // semitones
		bool transients = false;
		bool link_channels = false;

	  public:

		Batch_stats batch_stats;  // of the last process_payload: frames put / waits for their uploads

		static infra::Processor::Info get_processor_info();
		Processor::Info get_processor_info_non_static() const override { return get_processor_info(); }
		void draw_title() override;                         // bodies: draw-headless.cpp (the integrator keeps the reference's ImGui bodies instead)
		bool draw_content(bool readonly) override;
		std::vector<infra::Processor::Pin_attribute> get_pin_attributes() const override;
		void process_payload(
			const std::map<std::string, std::shared_ptr<infra::Processor::Product>>& input,
			const std::map<std::string, std::set<std::shared_ptr<infra::Processor::Product>>>& output,
			const std::atomic<bool>& stop_token,
			std::any& user_data
		) override;
		Json::Value serialize() const override;            // pitch (:495-500); algorithm, phase_lock, fft_size, formant, formant_shift, transients, link_channels when not the default
		void deserialize(const Json::Value& value) override;  // :502-505
	};

	// New node (registered as "audio_spectrum"): per channel, Hann-windowed fft_size-point r2c magnitude every hop
	// sample-frames (JSON keys "fft_size" = 256 ... 4096, a power of two, and "hop" = 1 ... fft_size; defaults 1024 / 256, which
	// are not written back).  Output stays an Audio_stream so the editor's pin type check passes: one FLTP frame per hop with
	// nb_samples = fft_size/2 + 1 (bins), plane c = |X_c[k]|, pts = start time of the analysed window.
	class Audio_spectrum : public infra::Processor
	{
	  public:

		static constexpr int default_fft_size = 1024, default_hop = 256;
		int fft_size = default_fft_size;
		int hop = default_hop;

		const void* last_context = nullptr;  // the nae_ctx its last process_payload ran on (every running node owns one: gpu-context.hpp); tests only

		static infra::Processor::Info get_processor_info();
		Processor::Info get_processor_info_non_static() const override { return get_processor_info(); }
		void draw_title() override;                         // bodies: draw-headless.cpp (the integrator keeps the reference's ImGui bodies instead)
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
